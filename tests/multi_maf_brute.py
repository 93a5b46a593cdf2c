"""Brute forces for the padded CIGARs of a star alignment (docs/design/04_30_block_maf_multi.md), straight from the definition: the sites
and widths of a group from a dictionary, the padded CIGAR of a chain by a walk over its reference bases, padded rows column by column,
and col0.  No GPU, nothing of ntsynt_amd."""
I, D, P, EQ, X = 1, 2, 6, 7, 8
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def len_a(entries):
    return sum(int(v) >> 4 for v in entries if int(v) & 15 in (EQ, X, D))


def len_b(entries):
    return sum(int(v) >> 4 for v in entries if int(v) & 15 in (EQ, X, I))


def widths(chains):
    "chains: (group, t0, entries) each.  {group: {slot: width}}: the longest I entry of the group in front of each reference base"
    out = {}
    for group, t0, entries in chains:
        p = int(t0)
        for v in entries:
            n, code = int(v) >> 4, int(v) & 15
            assert code in (I, D, EQ, X), code
            if code == I:
                sites = out.setdefault(group, {})
                sites[p] = max(sites.get(p, 0), n)
            else:
                p += n
    return out


def pad_chain(entries, t0, sites):
    "the padded CIGAR of one chain that begins at reference base t0; sites: {slot: width} of its group.  One reference base at a time"
    out, p, behind_own = [], int(t0), False
    for v in entries:
        n, code = int(v) >> 4, int(v) & 15
        if code == I:
            out.append(int(v))
            assert sites[p] >= n
            if sites[p] > n:
                out.append((sites[p] - n) << 4 | P)
            behind_own = True
            continue
        run = 0
        for base in range(p, p + n):
            if base in sites and not (base == p and behind_own):   # a foreign site in front of this base
                if run:
                    out.append(run << 4 | code)
                    run = 0
                out.append(sites[base] << 4 | P)
            run += 1
        out.append(run << 4 | code)
        p += n
        behind_own = False
    return out


def pad_all(chains, n_groups):
    """chains: (group, t0, entries) each, groups nondecreasing.  What Context.cigar_pad returns, as lists: (padded entries, pad_first,
    site_first, site_pos, site_w)"""
    sites = widths(chains)
    padded, pad_first = [], [0]
    for group, t0, entries in chains:
        padded += pad_chain(entries, t0, sites.get(group, {}))
        pad_first.append(len(padded))
    site_first, site_pos, site_w = [0], [], []
    for g in range(n_groups):
        for slot in sorted(sites.get(g, {})):
            site_pos.append(slot)
            site_w.append(sites[g][slot])
        site_first.append(len(site_pos))
    return padded, pad_first, site_first, site_pos, site_w


def col0(r0, sites, p):
    "the first column of slot p of a group that begins at reference base r0"
    return p - r0 + sum(w for q, w in sites.items() if q < p)


def columns_of(entries):
    return sum(int(v) >> 4 for v in entries)


def padded_rows(entries, target, query_as_read):
    "(row A, row B) of one padded chain, one column at a time: a P column is `-` in both rows and consumes nothing"
    row_a, row_b, i, j = [], [], 0, 0
    for v in entries:
        n, code = int(v) >> 4, int(v) & 15
        assert code in (I, D, P, EQ, X), code
        for _ in range(n):
            if code in (I, P):
                row_a.append("-")
            else:
                row_a.append(target[i])
                i += 1
            if code in (D, P):
                row_b.append("-")
            else:
                row_b.append(query_as_read[j])
                j += 1
    assert (i, j) == (len(target), len(query_as_read)), "the entries do not consume the two strings"
    return "".join(row_a), "".join(row_b)


def letters(seq):
    return "".join(ch if ch in "ACGT" else "N" for ch in seq.upper())


def reverse_complement(seq):
    return "".join(COMPLEMENT[ch] for ch in reversed(letters(seq)))


MAF_HEADER = "##maf version=1\n\n"


def core(entries):
    """(core entries, A bases cut off in front, B bases cut off in front); the core of a chain without = or X is None"""
    entries = [int(v) for v in entries]
    aligned = [i for i, v in enumerate(entries) if v & 15 in (EQ, X)]
    if not aligned:
        return None, 0, 0
    front = entries[:aligned[0]]
    return entries[aligned[0]:aligned[-1] + 1], len_a(front), len_b(front)


def cuts_of(chains):
    "the sorted distinct t0 and t1 of a group's chains: (t0, t1) each"
    return sorted({t for t0, t1 in chains for t in (t0, t1)})


def covering(chains, c, c_next):
    "the indices of the chains (t0, t1) that cover [c, c_next)"
    return [i for i, (t0, t1) in enumerate(chains) if t0 <= c and c_next <= t1]


def group_blocks(ref_name, ref_len, chains, sites):
    """the sub-blocks of one group as text, laid out one column at a time.  chains: dicts in row order -- row (>= 1), t0, t1, name,
    src_size, minus, start (of the core on the strand the `s` line counts on), row_a and row_b (its padded rows); sites: {slot: width}"""
    if not chains:
        return ""
    r0 = min(ch["t0"] for ch in chains)
    spans = [(ch["t0"], ch["t1"]) for ch in chains]
    out = []
    cuts = cuts_of(spans)
    for c, c_next in zip(cuts[:-1], cuts[1:]):
        lo, hi = col0(r0, sites, c), col0(r0, sites, c_next)
        reference, lines, rows_seen = None, [], []
        for i in covering(spans, c, c_next):
            ch = chains[i]
            base = col0(r0, sites, ch["t0"])
            assert len(ch["row_a"]) == len(ch["row_b"]) == col0(r0, sites, ch["t1"]) - base
            piece_a, piece_b, before, size = [], [], 0, 0
            for col, (a, b) in enumerate(zip(ch["row_a"], ch["row_b"])):
                if base + col < lo:
                    before += b != "-"
                elif base + col < hi:
                    piece_a.append(a)
                    piece_b.append(b)
                    size += b != "-"
            piece_a, piece_b = "".join(piece_a), "".join(piece_b)
            if reference is None:
                reference = piece_a
            assert piece_a == reference, "the covering chains disagree about the reference row"
            rows_seen.append(ch["row"])
            if size:
                lines.append(f"s {ch['name']} {ch['start'] + before} {size} {'-' if ch['minus'] else '+'} {ch['src_size']} {piece_b}\n")
        assert len(set(rows_seen)) == len(rows_seen) and rows_seen == sorted(rows_seen), "at most one covering chain per row, in row order"
        if not lines:
            continue
        size = sum(1 for a in reference if a != "-")
        out.append("a\n" + f"s {ref_name} {c} {size} + {ref_len} {reference}\n" + "".join(lines) + "\n")
    return "".join(out)


def table(groups):
    "groups: (ref_name, ref_len, chains, sites) each, in file order"
    return MAF_HEADER + "".join(group_blocks(*g) for g in groups)


def parse(text):
    "the sub-blocks of a multi-MAF file, read strictly: per block a list of (name, start, size, strand, src_size, row)"
    assert text.startswith(MAF_HEADER) and text.endswith("\n")
    blocks = []
    for chunk in text[len(MAF_HEADER):].split("\n\n")[:-1]:
        lines = chunk.split("\n")
        assert lines[0] == "a" and len(lines) >= 3, lines[0][:80]
        rows = []
        for ln in lines[1:]:
            s, name, start, size, strand, src, row = ln.split(" ")
            assert s == "s" and strand in "+-" and not set(row) - set("ACGTN-")
            assert int(size) == len(row) - row.count("-") > 0 and int(start) + int(size) <= int(src)
            rows.append((name, int(start), int(size), strand, int(src), row))
        assert len({len(r[5]) for r in rows}) == 1 and rows[0][3] == "+"
        blocks.append(rows)
    assert text[len(MAF_HEADER):] == "" or text.endswith("\n\n")
    return blocks

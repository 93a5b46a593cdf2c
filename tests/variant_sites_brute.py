"""The definitions of docs/design/04_32_block_variant_sites.md restated on the CPU, column by column: every chain is walked over its
columns, a dictionary keyed by (group, pos, kind, len, alt bytes) collects the carriers, the genotypes test every chain of every row.
Plain Python over lists and dictionaries; it shares no code with ntsynt_amd/assess.py and reads nothing of it.  Used by
tests/test_gpu_cigar_var_bases.py, tests/test_gpu_cigar_alleles.py, tests/test_gpu_cigar_alleles_order.py,
tests/test_variant_sites_host.py and tests/test_gpu_block_variant_sites.py."""

I, D, EQ, X = 1, 2, 7, 8
SNV, DEL, INS = 1, 2, 3
TYPES = {SNV: "snv", DEL: "del", INS: "ins"}


def variant_bytes(entries, row_a, row_b):
    "the ref and the alt bytes of one chain from its two aligned rows: row A at the X and D columns, row B at the X and I columns"
    ref, alt, col = [], [], 0
    for v in entries:
        code, size = v & 15, v >> 4
        for _ in range(size):
            if code in (X, D):
                ref.append(row_a[col])
            if code in (X, I):
                alt.append(row_b[col])
            col += 1
    assert col == len(row_a) == len(row_b)
    return "".join(ref), "".join(alt)


def byte_counts(entries):
    "(ref bytes, alt bytes) of one chain: its X + D and its X + I lengths"
    return (sum(v >> 4 for v in entries if v & 15 in (X, D)), sum(v >> 4 for v in entries if v & 15 in (X, I)))


def events(chains, alts):
    """chains: (group, t0, entries) each; alts[c]: chain c's alt bytes (bytes).  Returns per chain its events (pos, kind, len, alt bytes,
    ref offset, alt offset) in column order, the offsets counting in the concatenation over all chains"""
    out, ref_at, alt_at = [], 0, 0
    for (group, t0, entries), alt in zip(chains, alts):
        mine, p, a = [], t0, 0
        for v in entries:
            code, size = v & 15, v >> 4
            if code == X:
                for j in range(size):
                    mine.append((p + j, SNV, 1, bytes(alt[a + j:a + j + 1]), ref_at + j, alt_at + a + j))
                p, a, ref_at = p + size, a + size, ref_at + size
            elif code == D:
                mine.append((p, DEL, size, b"", ref_at, 0))
                p, ref_at = p + size, ref_at + size
            elif code == I:
                mine.append((p, INS, size, bytes(alt[a:a + size]), 0, alt_at + a))
                a += size
            else:
                assert code == EQ, code
                p += size
        assert a == len(alt), (a, len(alt))
        alt_at += a
        out.append(mine)
    return out


def alleles(chains, alts, n_groups):
    """What Context.cigar_alleles returns, as lists: (alleles, allele_first, carriers) with alleles = (pos, len, ref_off, alt_off,
    carrier_first, group, kind, n_carriers) tuples in the definition's order"""
    seen = {}
    for c, ((group, _, _), mine) in enumerate(zip(chains, events(chains, alts))):
        for pos, kind, size, text, ref_off, alt_off in mine:
            key = (group, pos, kind, size, text)
            if key not in seen:
                seen[key] = [ref_off, alt_off, []]            # (chains come in ascending order: the first one is the leader)
            seen[key][2].append(c)

    def order(key):
        group, pos, kind, size, text = key
        return (group, pos, kind, text[0] if kind == SNV else size, seen[key][2][0])
    out, carriers = [], []
    for key in sorted(seen, key=order):
        group, pos, kind, size, _ = key
        ref_off, alt_off, mine = seen[key]
        out.append((pos, size, ref_off, alt_off, len(carriers), group, kind, len(mine)))
        carriers += sorted(mine)
    first = [sum(1 for a in out if a[5] < g) for g in range(n_groups + 1)]
    return out, first, carriers


def genotypes(found, carriers, chains, chain_row, rows):
    "found: alleles' tuples; chains: (group, t0, entries); chain_row[c]: 1 .. rows[group].  One string per allele, every chain of every row tested"
    ends = [t0 + sum(v >> 4 for v in entries if v & 15 != I) for _, t0, entries in chains]
    out = []
    for pos, _, _, _, first, group, kind, n in found:
        mine = set(carriers[first:first + n])
        text = ""
        for row in range(1, rows[group] + 1):
            say = "."
            for c, (g, t0, _) in enumerate(chains):
                if g != group or chain_row[c] != row:
                    continue
                if c in mine:
                    say = "1"
                    break
                if (t0 < pos if kind == INS else t0 <= pos) and pos < ends[c]:
                    say = "0"
            text += say
        out.append(text)
    return out


def parameters(k, rate, band, max_len, max_edits, ends):
    text = f"# k {k}, rate {rate}, band {band}, max_len {max_len}, max_edits {max_edits}"
    if ends is not None:
        text += f", ends_max_len {ends[0]}, ends_max_edits {ends[1]}, ends_penalty {ends[2]}"
    return text


def table_text(groups, found, ref, alt, types, params):
    "groups: per group (block_id, genome, contig, start, end, rows); ref, alt: the byte buffers (bytes).  The text of <prefix>.block_variant_sites.tsv"
    lines = ["\t".join(("contig", "pos", "block_id", "genome", "type", "length", "ref", "alt", "rows", "aligned", "carriers", "genotypes"))]
    for (pos, size, ref_off, alt_off, _, group, kind, n), text in zip(found, types):
        block_id, genome, contig, _, _, rows = groups[group]
        ref_text = "-" if kind == INS else ref[ref_off:ref_off + size].decode()
        alt_text = "-" if kind == DEL else alt[alt_off:alt_off + size].decode()
        lines.append("\t".join(str(v) for v in (contig, pos, block_id, genome, TYPES[kind], size, ref_text, alt_text, rows,
                                                  sum(1 for ch in text if ch != "."), n, text)))
    lines.append(parameters(*params))
    return "\n".join(lines) + "\n"

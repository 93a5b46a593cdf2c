"""Brute force for nts_cigar_lift and the block lift (docs/design/04_23_block_lift.md), the definitions taken literally: a chain's CIGAR is
expanded to its columns, each with the (i, j) it stands at, and a query is answered by a walk over them; lift_from_paf makes the body of
<prefix>.block_lift.tsv from a PAF file alone, column by column.  No GPU, nothing of ntsynt_amd but the column names."""
CODE = {"I": 1, "D": 2, "=": 7, "X": 8}                       # BAM's codes
LETTER = {v: k for k, v in CODE.items()}


def columns(entries):
    """the columns of one chain: [(i, j, code, entry, off)] -- the column stands at base i of A and base j of B (the next base of a side
    it does not consume), belongs to entry `entry` of the chain (from 0) and is that entry's column number `off`"""
    out, i, j = [], 0, 0
    for e, v in enumerate(entries):
        length, code = int(v) >> 4, int(v) & 15
        assert code in LETTER and length > 0, (e, v)
        for off in range(length):
            out.append((i, j, code, e, off))
            i += code != CODE["I"]
            j += code != CODE["D"]
    return out, i, j


def lift(entries, side, pos, first=0):
    """the hit (pos, entry, off, code) of a query on one chain by a walk over its columns, or None for a position beyond the chain's end;
    first: the index of the chain's entry 0 in the whole CIGAR array"""
    cols, len_a, len_b = columns(entries)
    len_src, len_oth = (len_b, len_a) if side else (len_a, len_b)
    if pos > len_src:
        return None
    if pos == len_src:
        return (len_oth, first + len(entries), 0, 0)
    skips = CODE["D"] if side else CODE["I"]                  # the kind of column that does not consume the source side
    for i, j, code, e, _ in cols:
        src, oth = (j, i) if side else (i, j)
        if code != skips and src == pos:
            before = sum(int(v) >> 4 for v in entries[:e] if int(v) & 15 != skips)       # Psrc[e]
            return (oth, first + e, pos - before, code)
    raise AssertionError("a base of the chain in no column")


class Walker:
    "the columns of one chain, expanded once: the same answers as lift() for many queries"

    def __init__(self, entries, first=0):
        self.cols, self.len_a, self.len_b = columns(entries)
        self.first, self.n = first, len(entries)
        self.at = ({}, {})                                    # per side: source base -> its column
        for c, (i, j, code, _, _) in enumerate(self.cols):
            if code != CODE["I"]:
                self.at[0][i] = c
            if code != CODE["D"]:
                self.at[1][j] = c

    def lift(self, side, pos):
        len_src, len_oth = (self.len_b, self.len_a) if side else (self.len_a, self.len_b)
        if pos > len_src:
            return None
        if pos == len_src:
            return (len_oth, self.first + self.n, 0, 0)
        i, j, code, e, off = self.cols[self.at[side][pos]]
        return ((i if side else j), self.first + e, off, code)


def swap_sides(entries):
    "the same alignment with the roles of A and B exchanged: I and D swapped"
    other = {CODE["I"]: CODE["D"], CODE["D"]: CODE["I"]}
    return [(int(v) >> 4) << 4 | other.get(int(v) & 15, int(v) & 15) for v in entries]


def parse_cigar(text):
    "the entries len << 4 | code of an =/X/I/D CIGAR string"
    out, number = [], ""
    for ch in text:
        if ch.isdigit():
            number += ch
        else:
            out.append(int(number) << 4 | CODE[ch])
            number = ""
    assert number == ""
    return out


def read_bed_lines(text):
    "[(contig, start, end, name)] of a BED text, comment lines left out"
    out = []
    for line in text.splitlines():
        if not line.strip() or line.startswith(("#", "track", "browser")):
            continue
        f = line.split("\t")
        out.append((f[0], int(f[1]), int(f[2]), f[3] if len(f) > 3 else "."))
    return out


def lift_from_paf(paf_text, bed, source):
    """the lines of <prefix>.block_lift.tsv between header and footer, from the PAF text of the same run: bed = [(contig, start, end,
    name)], source = the genome the intervals lie on.  Every record in which `source` is the target
    (tg) or the query (qg) is expanded to its columns; the columns of the interval's bases are looked up one by one.  Also returns
    per line whether both its end columns are `=` (for the base comparison of the test)."""
    from ntsynt_amd.assess import LIFT_COLUMNS as columns_of
    records = []
    for line in paf_text.splitlines():
        f = line.split("\t")
        tags = {t[:5]: t[5:] for t in f[12:]}
        if source not in (tags["tg:Z:"], tags["qg:Z:"]):
            continue
        side = 0 if tags["tg:Z:"] == source else 1
        records.append(dict(side=side, flip=f[4] == "-", q=f[0], q0=int(f[2]), q1=int(f[3]), t=f[5], t0=int(f[7]), t1=int(f[8]), block=tags["bi:i:"],
                            other=tags["qg:Z:"] if side == 0 else tags["tg:Z:"], ch=int(tags["ch:i:"]), walker=Walker(parse_cigar(tags["cg:Z:"]))))
    lines, in_equal = [], []
    for contig, start, end, name in bed:
        head = [source, contig, start, end, name]
        found = False
        for r in records:
            s0, s1, mine = (r["q0"], r["q1"], r["q"]) if r["side"] else (r["t0"], r["t1"], r["t"])
            lo, hi = max(start, s0), min(end, s1)
            if mine != contig or lo >= hi:
                continue
            found = True
            mirrored = r["side"] == 1 and r["flip"]           # the query's bases run backwards along the chain
            local = [s1 - 1 - p if mirrored else p - s0 for p in range(lo, hi)]
            hits = [r["walker"].lift(r["side"], u) for u in (min(local), max(local))]
            v_lo = hits[0][0]
            v_hi = hits[1][0] + (1 if hits[1][3] in (CODE["="], CODE["X"]) else 0)
            assert v_lo <= v_hi
            if r["side"] == 1:
                to = (r["t"], r["t0"] + v_lo, r["t0"] + v_hi)
            elif r["flip"]:
                to = (r["q"], r["q1"] - v_hi, r["q1"] - v_lo)
            else:
                to = (r["q"], r["q0"] + v_lo, r["q0"] + v_hi)
            row = dict(zip(columns_of, head + [r["block"], r["other"], to[0], to[1], to[2], "-" if r["flip"] else "+", r["ch"], lo, hi,
                                               "full" if (lo, hi) == (start, end) else "partial"]))
            lines.append("\t".join(str(row[c]) for c in columns_of))
            in_equal.append(all(h[3] == CODE["="] for h in hits))
        if not found:
            lines.append("\t".join(str(v) for v in head + ["."] * 9 + ["unmapped"]))
            in_equal.append(False)
    return lines, in_equal

"""Brute force for nts_cigar_lift_pairs and the joined lift (docs/design/04_27_lift_joined.md), the definition taken literally: the columns
of a pair's linked chains are expanded and put one behind the other in link order, each with the oriented bases of A and B it stands at
(tests/lift_brute.columns plus the link's a0 / b0); an open stretch between two chains has no column.  A range is answered by a walk:
the first and the last column that hold a source base of [lo, hi) are looked up, every column from the one to the other is counted one
by one, runs are counted on the COLUMN sequence with a new run at every chain's first column, and the open bases are added up link by
link.  joined_from_paf makes the body of <prefix>.block_lift_joined.tsv / <prefix>.block_windows_joined.tsv from a PAF file alone.  No
GPU, nothing of ntsynt_amd but the column names."""
from tests import lift_brute as LB
from tests.lift_stats_brute import identity_text

CODE = LB.CODE
FIELDS = ("src_lo", "src_hi", "oth_lo", "oth_hi", "eq", "x", "src_gap", "oth_gap", "src_open", "oth_open", "src_gaps", "oth_gaps", "link_lo", "link_hi",
          "n_links")
NONE = (0,) * len(FIELDS)


class PairWalker:
    "the columns of one pair, expanded once: stats for many ranges.  links: [(entries, a0, b0)] in link order; first_link: the index of links[0]"

    def __init__(self, links, first_link=0):
        import numpy as np
        a, b, code, link, run = [], [], [], [], []
        self.spans, self.first_link = [], first_link
        for k, (entries, a0, b0) in enumerate(links):
            cols, len_a, len_b = LB.columns(entries)
            self.spans.append((a0, a0 + len_a, b0, b0 + len_b))
            for c, (i, j, kind, _, _) in enumerate(cols):
                # a run of one kind ends where the kind changes and where the chain ends
                run.append((run[-1] if run else 0) + (1 if c == 0 or kind != cols[c - 1][2] else 0))
                a.append(a0 + i)
                b.append(b0 + j)
                code.append(kind)
                link.append(k)
        self.a, self.b, self.code, self.link, self.run = (np.array(v, dtype=np.int64) for v in (a, b, code, link, run))

    def stats(self, side, lo, hi):
        "the record of the bases lo .. hi - 1 of `side`, as a tuple in the order of FIELDS; None for a range that is not valid"
        import numpy as np
        if side not in (0, 1) or not lo < hi < 2 ** 63:
            return None
        src, oth = (self.b, self.a) if side else (self.a, self.b)
        src_only, oth_only = (CODE["I"], CODE["D"]) if side else (CODE["D"], CODE["I"])
        holds = np.flatnonzero((self.code != oth_only) & (src >= lo) & (src < hi))      # the columns that hold a base of the range
        if holds.size == 0:
            return NONE
        c_lo, c_hi = int(holds[0]), int(holds[-1])
        counted, of_run = self.code[c_lo:c_hi + 1], self.run[c_lo:c_hi + 1]             # every column from c_lo to c_hi, the two included
        count = {code: int(np.count_nonzero(counted == code)) for code in CODE.values()}
        runs = {code: len(set(of_run[counted == code].tolist())) for code in (src_only, oth_only)}
        link_lo, link_hi = int(self.link[c_lo]), int(self.link[c_hi])
        src_open = oth_open = 0
        for k in range(link_lo, link_hi):                     # the open stretch behind link k
            a0, a1, b0, b1 = self.spans[k]
            n0, _, m0, _ = self.spans[k + 1]
            src_open += (m0 - b1) if side else (n0 - a1)
            oth_open += (n0 - a1) if side else (m0 - b1)
        oth_hi = int(oth[c_hi]) + (int(self.code[c_hi]) in (CODE["="], CODE["X"]))
        return (int(src[c_lo]), int(src[c_hi]) + 1, int(oth[c_lo]), oth_hi, count[CODE["="]], count[CODE["X"]], count[src_only], count[oth_only], src_open,
                oth_open, runs[src_only], runs[oth_only], self.first_link + link_lo, self.first_link + link_hi, link_hi - link_lo + 1)


def identities_hold(record):
    "the two length identities of a record (a tuple in the order of FIELDS)"
    src_lo, src_hi, oth_lo, oth_hi, eq, x, src_gap, oth_gap, src_open, oth_open = record[:10]
    return eq + x + src_gap + src_open == src_hi - src_lo and eq + x + oth_gap + oth_open == oth_hi - oth_lo


def paf_pairs(paf_text, source):
    """the pairs of a PAF text in which `source` takes part, in file order: per (block, target genome, query genome) its records as
    dicts, ascending by ch"""
    pairs = {}
    for line in paf_text.splitlines():
        f = line.split("\t")
        tags = {t[:5]: t[5:] for t in f[12:]}
        if source not in (tags["tg:Z:"], tags["qg:Z:"]):
            continue
        side = 0 if tags["tg:Z:"] == source else 1
        rec = dict(side=side, flip=f[4] == "-", q=f[0], q0=int(f[2]), q1=int(f[3]), t=f[5], t0=int(f[7]), t1=int(f[8]), block=tags["bi:i:"],
                   other=tags["qg:Z:"] if side == 0 else tags["tg:Z:"], ch=int(tags["ch:i:"]), entries=LB.parse_cigar(tags["cg:Z:"]))
        pairs.setdefault((tags["bi:i:"], tags["tg:Z:"], tags["qg:Z:"]), []).append(rec)
    return [sorted(records, key=lambda r: r["ch"]) for records in pairs.values()]


def joined_from_paf(paf_text, bed, source):
    """the lines of <prefix>.block_lift_joined.tsv (or block_windows_joined.tsv) between header and footer, from the PAF text of the same
    run: bed = [(contig, start, end, name)], source = the genome the intervals lie on.  The records of a pair are placed on a common
    axis per genome -- the target forwards from 0, the query forwards for `+` and mirrored at the largest query end for `-`, so that both
    ascend with ch -- and walked as one column sequence (PairWalker); the interval's bases are mapped onto the source axis one end at a
    time."""
    from ntsynt_amd.assess import LIFT_JOINED_COLUMNS as columns_of
    walkers = []
    for records in paf_pairs(paf_text, source):
        r0 = records[0]
        top = max(r["q1"] for r in records)                   # a `-` pair: oriented query offset = top - forward position
        links = [(r["entries"], r["t0"], top - r["q1"] if r["flip"] else r["q0"]) for r in records]
        walkers.append((r0, top, PairWalker(links), [r["ch"] for r in records]))
    lines = []
    for contig, start, end, name in bed:
        head = [source, contig, start, end, name]
        found = False
        for r0, top, walker, chs in walkers:
            side, flip = r0["side"], r0["flip"]
            if (r0["q"] if side else r0["t"]) != contig:
                continue
            mirrored = side == 1 and flip
            lo, hi = (top - end, top - start) if mirrored else (start, end)
            if hi <= 0:
                continue
            got = walker.stats(side, max(lo, 0), hi)
            if got is None or got[14] == 0:
                continue
            found = True
            assert identities_hold(got)
            src_lo, src_hi, oth_lo, oth_hi, eq, x, src_gap, oth_gap, src_open, oth_open, src_gaps, oth_gaps, link_lo, link_hi, n_links = got
            s = (top - src_hi, top - src_lo) if mirrored else (src_lo, src_hi)
            to = (top - oth_hi, top - oth_lo) if side == 0 and flip else (oth_lo, oth_hi)
            columns = eq + x + src_gap + oth_gap
            row = dict(zip(columns_of, head + [r0["block"], r0["other"], r0["t"] if side else r0["q"], to[0], to[1], "-" if flip else "+", n_links, chs[link_lo],
                                               chs[link_hi], s[0], s[1], eq, x, src_gap, oth_gap, src_gaps, oth_gaps, src_open, oth_open, columns,
                                               identity_text(eq, columns), "full" if s == (start, end) else "partial"]))
            lines.append("\t".join(str(row[c]) for c in columns_of))
        if not found:
            lines.append("\t".join(str(v) for v in head + ["."] * (len(columns_of) - 6) + ["unmapped"]))
    return lines

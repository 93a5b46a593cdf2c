"""Brute force for nts_cigar_lift_stats and the lift identity (docs/design/04_25_lift_identity.md), the definition taken literally: a
chain's CIGAR is expanded to its columns (tests/lift_brute.columns), the columns of the range's first and last base are looked up, and
every column from the one to the other is counted one by one; runs are counted on the COLUMN sequence, not on entries.
identity_from_paf makes the body of <prefix>.block_lift_identity.tsv / <prefix>.block_windows.tsv from a PAF file alone.  No GPU, nothing
of ntsynt_amd but the column names."""
from tests import lift_brute as LB

CODE = LB.CODE
FIELDS = ("oth_lo", "oth_hi", "eq", "x", "src_gap", "oth_gap", "src_gaps", "oth_gaps")


class Counter:
    "the columns of one chain, expanded once: range_stats for many ranges"

    def __init__(self, entries):
        import numpy as np
        self.cols, self.len_a, self.len_b = LB.columns(entries)
        run, self.at = [], ({}, {})                           # per column the number of its maximal run of one kind; per side: source base -> its column
        for c, (i, j, code, _, _) in enumerate(self.cols):
            run.append(0 if c == 0 else run[-1] + (code != self.cols[c - 1][2]))
            if code != CODE["I"]:
                self.at[0][i] = c
            if code != CODE["D"]:
                self.at[1][j] = c
        self.code, self.run = np.array([c[2] for c in self.cols], dtype=np.int64), np.array(run, dtype=np.int64)

    def stats(self, side, lo, hi):
        "the record of the bases lo .. hi - 1 of `side`, as a tuple in the order of FIELDS; None for a range that is not valid"
        len_src = self.len_b if side else self.len_a
        if side not in (0, 1) or not lo < hi <= len_src:
            return None
        src_only, oth_only = (CODE["I"], CODE["D"]) if side else (CODE["D"], CODE["I"])
        c_lo, c_hi = self.at[side][lo], self.at[side][hi - 1]
        import numpy as np
        counted, of_run = self.code[c_lo:c_hi + 1], self.run[c_lo:c_hi + 1]             # every column from c_lo to c_hi, the two included
        count = {code: int(np.count_nonzero(counted == code)) for code in CODE.values()}
        runs = {code: set(of_run[counted == code].tolist()) for code in (src_only, oth_only)}
        i, j, code, _, _ = self.cols[c_lo]
        oth_lo = i if side else j
        i, j, code, _, _ = self.cols[c_hi]
        oth_hi = (i if side else j) + (code in (CODE["="], CODE["X"]))
        return (oth_lo, oth_hi, count[CODE["="]], count[CODE["X"]], count[src_only], count[oth_only], len(runs[src_only]), len(runs[oth_only]))


def range_stats(entries, side, lo, hi):
    "one range of one chain by a walk over its columns (Counter.stats)"
    return Counter(entries).stats(side, lo, hi)


def identity_text(matches, columns):
    "10^6 matches // columns as d.dddddd"
    v = (10 ** 6 * matches) // columns
    return f"{v // 10 ** 6}.{v % 10 ** 6:06d}"


def identity_from_paf(paf_text, bed, source):
    """the lines of <prefix>.block_lift_identity.tsv (or block_windows.tsv) between header and footer, from the PAF text of the same run:
    bed = [(contig, start, end, name)], source = the genome the intervals lie on.  As lift_brute.lift_from_paf: every record in which
    `source` is the target or the query is expanded to its columns; the interval's bases are mapped to chain-local offsets one by one and
    the columns between the smallest and the largest are counted."""
    from ntsynt_amd.assess import LIFT_IDENTITY_COLUMNS as columns_of
    records = []
    for line in paf_text.splitlines():
        f = line.split("\t")
        tags = {t[:5]: t[5:] for t in f[12:]}
        if source not in (tags["tg:Z:"], tags["qg:Z:"]):
            continue
        side = 0 if tags["tg:Z:"] == source else 1
        records.append(dict(side=side, flip=f[4] == "-", q=f[0], q0=int(f[2]), q1=int(f[3]), t=f[5], t0=int(f[7]), t1=int(f[8]), block=tags["bi:i:"],
                            other=tags["qg:Z:"] if side == 0 else tags["tg:Z:"], ch=int(tags["ch:i:"]), counter=Counter(LB.parse_cigar(tags["cg:Z:"]))))
    lines = []
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
            local = [s1 - 1 - p if mirrored else p - s0 for p in (lo, hi - 1)]
            v_lo, v_hi, eq, x, src_gap, oth_gap, src_gaps, oth_gaps = r["counter"].stats(r["side"], min(local), max(local) + 1)
            assert v_lo <= v_hi and eq + x + src_gap == hi - lo and eq + x + oth_gap == v_hi - v_lo
            if r["side"] == 1:
                to = (r["t"], r["t0"] + v_lo, r["t0"] + v_hi)
            elif r["flip"]:
                to = (r["q"], r["q1"] - v_hi, r["q1"] - v_lo)
            else:
                to = (r["q"], r["q0"] + v_lo, r["q0"] + v_hi)
            columns = eq + x + src_gap + oth_gap
            row = dict(zip(columns_of, head + [r["block"], r["other"], to[0], to[1], to[2], "-" if r["flip"] else "+", r["ch"], lo, hi, eq, x, src_gap, oth_gap,
                                               src_gaps, oth_gaps, columns, identity_text(eq, columns), "full" if (lo, hi) == (start, end) else "partial"]))
            lines.append("\t".join(str(row[c]) for c in columns_of))
        if not found:
            lines.append("\t".join(str(v) for v in head + ["."] * (len(columns_of) - 6) + ["unmapped"]))
    return lines

"""Brute forces for the block variants (docs/design/04_17_block_variants.md), straight from the definitions: the full Levenshtein
table, the walk that picks the canonical script, the merging of ops into events, the coordinates and the file text.  No GPU, nothing
of ntsynt_amd.assess."""
import numpy as np

from tests import identity_brute as B

SUB, DEL, INS = 1, 2, 3
NO_BASE = 0xFF
CODE = {65: 0, 67: 1, 71: 2, 84: 3}                          # ASCII -> the device's base codes
COLUMNS = ("block_id", "genome_a", "contig_a", "pos_a", "genome_b", "contig_b", "pos_b", "orientation", "type", "length", "seq_a", "seq_b")


def table(a, b):
    "T[i][j] = the unit-cost edit distance of a[:i] and b[:j], the whole table"
    a, b = np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint8)
    ramp = np.arange(b.size + 1, dtype=np.int32)
    t = np.empty((a.size + 1, b.size + 1), dtype=np.int32)
    t[0] = ramp
    for i in range(a.size):
        best = np.empty(b.size + 1, dtype=np.int32)
        best[0] = i + 1
        np.minimum(t[i, 1:] + 1, t[i, :-1] + (b != a[i]), out=best[1:])
        t[i + 1] = np.minimum.accumulate(best - ramp) + ramp   # (the steps along the row, as identity_brute.levenshtein takes them)
    return t


def script(a, b):
    """the canonical script of two ASCII uint8 arrays: (op, p, q) in ascending path order.  The walk from (n, m): a match first,
    then SUB, then DEL, else INS"""
    a, b = np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint8)
    if a.size == b.size and (a == b).all():
        return []
    t = table(a, b)
    i, j, out = a.size, b.size, []
    while i > 0 or j > 0:
        if i > 0 and j > 0 and a[i - 1] == b[j - 1]:
            assert t[i - 1][j - 1] == t[i][j]
            i, j = i - 1, j - 1
        elif i > 0 and j > 0 and t[i - 1][j - 1] + 1 == t[i][j]:
            out.append((SUB, i - 1, j - 1))
            i, j = i - 1, j - 1
        elif i > 0 and t[i - 1][j] + 1 == t[i][j]:
            out.append((DEL, i - 1, j))
            i -= 1
        else:
            assert j > 0 and t[i][j - 1] + 1 == t[i][j]
            out.append((INS, i, j - 1))
            j -= 1
    assert len(out) == t[a.size][b.size]
    return out[::-1]


def apply_script(a, ops):
    "string A with the ops (op, p, q, base of B or None) applied: string B"
    a = list(np.asarray(a, dtype=np.uint8).tolist())
    out, at = [], 0
    for op, p, _, base_b in ops:
        assert p >= at, "ops out of path order"
        out += a[at:p]
        at = p
        if op == SUB:
            out.append(base_b)
            at += 1
        elif op == DEL:
            at += 1
        else:
            out.append(base_b)
    return np.array(out + a[at:], dtype=np.uint8)


def op_records(seg_index, a, b):
    "the nts_edit_op fields (seg, p, q, op, base_a, base_b) of one segment's canonical script; a, b ASCII, b oriented"
    return [(seg_index, p, q, op, CODE[int(a[p])] if op != INS else NO_BASE, CODE[int(b[q])] if op != DEL else NO_BASE) for op, p, q in script(a, b)]


def events(ops, a, b):
    "the events of one segment: (type, p0, q0, bases of A, bases of B), maximal runs of adjacent ops; a, b ASCII, b oriented"
    out = []
    for op, p, q in ops:
        last = out[-1] if out else None
        if op == DEL and last and last[0] == "del" and p == last[1] + len(last[3]) and q == last[2]:
            last[3] += chr(a[p])
        elif op == INS and last and last[0] == "ins" and p == last[1] and q == last[2] + len(last[4]):
            last[4] += chr(b[q])
        else:
            out.append([{SUB: "snv", DEL: "del", INS: "ins"}[op], p, q, chr(a[p]) if op != INS else "", chr(b[q]) if op != DEL else ""])
    return out


def place(event, x, y_lo, start_a, start_b, len_b, flipped):
    "(pos_a, pos_b) of an event of a segment at (x, y_lo) of intervals that start at start_a / start_b, B's of len_b bases"
    _, p0, q0, _, seq_b = event
    y = y_lo + q0
    return start_a + x + p0, (start_b + len_b - y - len(seq_b)) if flipped else start_b + y


def brute_file(table_rows, genomes, hash_all, k, rate, band, max_len):
    """the whole variants file and per pair the number of ops.  Arguments as identity_brute.brute_file, whose anchors, segments and
    distances it takes (a table in which no block has two lines of one genome).  Returns (text, identity text, {(block, genome_a,
    genome_b): [ops, [event rows]]})"""
    id_text, facts = B.brute_file(table_rows, genomes, hash_all, k, rate, band, max_len)
    line_of = {(r.block_id, r.genome): r for r in table_rows}
    assert len(line_of) == len(table_rows)
    text, per_pair = ["\t".join(COLUMNS)], {}
    for (block, name_a, name_b), (row, segs) in facts.items():
        ra, rb = line_of[(block, name_a)], line_of[(block, name_b)]
        seq_a, seq_b = genomes[name_a][ra.contig], genomes[name_b][rb.contig]
        start_a, start_b = min(max(ra.start, 0), seq_a.size), min(max(rb.start, 0), seq_b.size)
        len_a, len_b = row["length_a"], row["length_b"]
        flipped = row["orientation"] == "-"
        found, n_ops = [], 0
        for seg, d in segs:
            if d >= B.INVALID:
                continue
            a, b = B.strings_of(seq_a, seq_b, (start_a, len_a), (start_b, len_b), flipped, seg)
            ops = script(a, b)
            assert len(ops) == d
            n_ops += len(ops)
            for ev in events(ops, a, b):
                pos_a, pos_b = place(ev, seg[1], seg[3], start_a, start_b, len_b, flipped)
                found.append((pos_a, pos_b, ev[0], max(len(ev[3]), len(ev[4])), ev[3] or "-", ev[4] or "-"))
        found.sort(key=lambda e: e[0])                        # (stable: script order within one pos_a)
        rows = ["\t".join(str(v) for v in (block, name_a, ra.contig, e[0], name_b, rb.contig, e[1], row["orientation"], e[2], e[3], e[4], e[5]))
                for e in found]
        text += rows
        per_pair[(block, name_a, name_b)] = [n_ops, rows]
    text.append(f"# k {k}, rate {rate}, band {band}, max_len {max_len}")
    return "\n".join(text) + "\n", id_text, per_pair

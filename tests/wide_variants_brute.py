"""Brute force for the block wide variants (docs/design/04_19_block_wide_variants.md), straight from the definitions: the script set of
nts_edit_wide_script from the final distances of tests/wide_brute.py, every member's canonical script from the full table and walk of
tests/variants_brute.py, and the whole expected file from wide_brute.brute_file_wide's segments.  No GPU, nothing of
ntsynt_amd.assess."""
from tests import identity_brute as B
from tests import variants_brute as V
from tests import wide_brute as W


def in_script_set(seg, final, band):
    "a distance that nts_edit_script does not take: kind offband, or a candidate with D + |dy - dx| > 2 band + 1"
    _, _, dx, _, dy, kind = seg
    if final >= B.INVALID:
        return False
    return kind == B.OFFBAND or (kind == B.CANDIDATE and final + abs(dy - dx) > 2 * band + 1)


def expected_ops(seq_a, seq_b, ivs_a, ivs_b, flip, segs, final, band):
    """(ops, first, members): the nts_edit_op fields (seg, p, q, op, base_a, base_b) of every member of the script set one behind the
    other, first[i] .. first[i + 1] the ops of segment i (equal for what is no member), the members' indices"""
    ops, first, members = [], [0], []
    for q, seg in enumerate(segs):
        if in_script_set(seg, final[q], band):
            a, b = B.strings_of(seq_a, seq_b, ivs_a[seg[0]], ivs_b[seg[0]], flip[seg[0]], seg)
            mine = V.op_records(q, a, b)
            assert len(mine) == final[q] >= 1, (q, len(mine), final[q])
            ops += mine
            members.append(q)
        first.append(len(ops))
    return ops, first, members


def brute_file(table_rows, genomes, hash_all, k, rate, band, max_len, max_edits):
    """the whole wide variants file.  Arguments as wide_brute.brute_file_wide, whose segments and final distances it takes.  Returns
    (text, identity text with E, {(block, genome_a, genome_b): [ops, [event rows], [(segment, D, inserted bases, deleted bases, first
    and last pos_a an event of the segment can have)]]})"""
    id_text, facts, _ = W.brute_file_wide(table_rows, genomes, hash_all, k, rate, band, max_len, max_edits)
    line_of = {(r.block_id, r.genome): r for r in table_rows}
    assert len(line_of) == len(table_rows)
    text, per_pair = ["\t".join(V.COLUMNS)], {}
    for (block, name_a, name_b), (row, segs) in facts.items():
        ra, rb = line_of[(block, name_a)], line_of[(block, name_b)]
        seq_a, seq_b = genomes[name_a][ra.contig], genomes[name_b][rb.contig]
        start_a, start_b = min(max(ra.start, 0), seq_a.size), min(max(rb.start, 0), seq_b.size)
        len_a, len_b = row["length_a"], row["length_b"]
        flipped = row["orientation"] == "-"
        found, n_ops, stretches = [], 0, []
        for seg, d in segs:
            if d >= B.INVALID:
                continue
            a, b = B.strings_of(seq_a, seq_b, (start_a, len_a), (start_b, len_b), flipped, seg)
            ops = V.script(a, b)
            assert len(ops) == d
            n_ops += len(ops)
            stretches.append((seg, d, sum(op == V.INS for op, _, _ in ops), sum(op == V.DEL for op, _, _ in ops), start_a + seg[1],
                              start_a + seg[1] + seg[2]))
            for ev in V.events(ops, a, b):
                pos_a, pos_b = V.place(ev, seg[1], seg[3], start_a, start_b, len_b, flipped)
                found.append((pos_a, pos_b, ev[0], max(len(ev[3]), len(ev[4])), ev[3] or "-", ev[4] or "-"))
        found.sort(key=lambda e: e[0])                        # (stable: script order within one pos_a)
        rows = ["\t".join(str(v) for v in (block, name_a, ra.contig, e[0], name_b, rb.contig, e[1], row["orientation"], e[2], e[3], e[4], e[5]))
                for e in found]
        assert n_ops == row["edits"]
        text += rows
        per_pair[(block, name_a, name_b)] = [n_ops, rows, stretches]
    text.append(f"# k {k}, rate {rate}, band {band}, max_len {max_len}, max_edits {max_edits}")
    return "\n".join(text) + "\n", id_text, per_pair

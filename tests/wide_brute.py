"""Brute force for the wide pass of the block identity (docs/design/04_18_block_identity_wide.md), straight from the definitions: the
full unrestricted (dx + 1) x (dy + 1) table of tests/identity_brute.py per segment and the precedence of the kinds with E > 0 --
backward, long, offband (|dy - dx| > E), invalid, overband (D > E), aligned.  No GPU, nothing of ntsynt_amd.assess."""
import numpy as np

from tests import identity_brute as B


def valid_bases():
    ok = np.zeros(256, dtype=bool)
    ok[list(B.COMPLEMENT)] = True
    return ok


def in_work_set(seg, narrow, max_edits):
    "what nts_edit_wide looks at again: offband with |dy - dx| <= E, and candidates the narrow pass called overband"
    _, _, dx, _, dy, kind = seg
    return (kind == B.OFFBAND and narrow == B.PASSED and abs(dy - dx) <= max_edits) or (kind == B.CANDIDATE and narrow == B.OVERBAND)


def wide_result(a, b, max_edits, ok=None):
    "INVALID, the unrestricted distance D <= E, or OVERBAND"
    ok = valid_bases() if ok is None else ok
    if not (ok[a].all() and ok[b].all()):
        return B.INVALID
    d = B.levenshtein(a, b)
    return d if d <= max_edits else B.OVERBAND


def brute_wide(seq_a, seq_b, ivs_a, ivs_b, flip, segs, band, max_edits):
    """(narrow per-segment results = nts_edit_segments' dist_out, final per-segment results, per-interval dicts over the final results,
    the work set's indices).  segs carry the kind nts_iv_anchor_segments gives them with `band`; ivs: (absolute start, length) per
    interval of A and of its mate."""
    assert 2 * band + 1 <= max_edits <= 1023
    ok = valid_bases()
    narrow, final, work = [], [], []
    per_iv = [dict(aligned_a=0, aligned_b=0, edits=0, segments=0, aligned=0, backward=0, too_long=0, offband=0, invalid=0, overband=0)
              for _ in ivs_a]
    for q, seg in enumerate(segs):
        iv, _, dx, _, dy, kind = seg
        row = per_iv[iv]
        row["segments"] += 1
        if kind in (B.BACKWARD, B.LONG):
            row["backward" if kind == B.BACKWARD else "too_long"] += 1
            narrow.append(B.PASSED)
            final.append(B.PASSED)
            continue
        if kind not in (B.CANDIDATE, B.OFFBAND):
            narrow.append(B.NOT_CANDIDATE)
            final.append(B.NOT_CANDIDATE)
            continue
        if kind == B.OFFBAND and abs(dy - dx) > max_edits:
            row["offband"] += 1
            narrow.append(B.PASSED)
            final.append(B.PASSED)
            continue
        a, b = B.strings_of(seq_a, seq_b, ivs_a[iv], ivs_b[iv], flip[iv], seg)
        d = wide_result(a, b, max_edits, ok)
        if kind == B.OFFBAND:
            narrow.append(B.PASSED)
        elif d == B.INVALID:
            narrow.append(B.INVALID)
        elif d == B.OVERBAND or (d + abs(dy - dx)) // 2 > band:
            narrow.append(B.OVERBAND)
        else:
            narrow.append(d)
        if in_work_set(seg, narrow[-1], max_edits):
            work.append(q)
        final.append(d)
        if d == B.INVALID:
            row["invalid"] += 1
        elif d == B.OVERBAND:
            row["overband"] += 1
        else:
            row["aligned"] += 1
            row["aligned_a"] += dx
            row["aligned_b"] += dy
            row["edits"] += d
    return narrow, final, per_iv, work


def brute_file_wide(table, genomes, hash_all, k, rate, band, max_len, max_edits):
    """the whole file with max_edits = E > 0, from identity_brute.brute_file's segments: a narrow distance stands (D <= 2 band + 1 <= E),
    so do invalid, backward and long; an offband segment with |dy - dx| <= E and a narrow overband get the full table.  Returns (text,
    facts) as brute_file does, the results being the final ones, and the narrow text."""
    narrow_text, narrow_facts = B.brute_file(table, genomes, hash_all, k, rate, band, max_len)
    assert len(narrow_facts) == len(narrow_text.splitlines()) - 2, "two pairs of one block share their genomes: the facts do not tell them apart"
    ok = valid_bases()
    line_of = {}
    for r in table:
        assert (r.block_id, r.genome) not in line_of
        line_of[(r.block_id, r.genome)] = r
    text, facts = [narrow_text.splitlines()[0]], {}
    for (b, name_a, name_b), (row, results) in narrow_facts.items():
        ra, rb = line_of[(b, name_a)], line_of[(b, name_b)]
        seq_a, seq_b = genomes[name_a][ra.contig], genomes[name_b][rb.contig]
        clip = lambda r, n: (min(max(r.start, 0), n), max(min(max(r.end, 0), n) - min(max(r.start, 0), n), 0))      # noqa: E731
        iv_a, iv_b = clip(ra, seq_a.size), clip(rb, seq_b.size)
        assert (iv_a[1], iv_b[1]) == (row["length_a"], row["length_b"])
        new = dict(row, aligned=0, aligned_a=0, aligned_b=0, edits=0, offband=0, invalid=0, overband=0)
        out = []
        for seg, narrow in results:
            d = narrow
            if in_work_set(seg, narrow, max_edits):
                d = wide_result(*B.strings_of(seq_a, seq_b, iv_a, iv_b, ra.strand != rb.strand, seg), max_edits, ok)
            out.append((seg, d))
            if d < B.INVALID:
                assert d <= max_edits
                new["aligned"] += 1
                new["aligned_a"] += seg[2]
                new["aligned_b"] += seg[4]
                new["edits"] += d
            elif d == B.INVALID:
                new["invalid"] += 1
            elif d == B.OVERBAND:
                new["overband"] += 1
            elif seg[5] == B.OFFBAND:
                new["offband"] += 1
        assert new["aligned"] + new["invalid"] + new["overband"] + new["offband"] + new["backward"] + new["long"] == new["segments"]
        text.append(B.format_row(new))
        facts[(b, name_a, name_b)] = (new, out)
    text.append(f"# k {k}, rate {rate}, band {band}, max_len {max_len}, max_edits {max_edits}")
    return "\n".join(text) + "\n", facts, narrow_text

"""Brute forces for the block MAF (docs/design/04_29_block_maf.md), straight from the definition: the two rows of a CIGAR walked column by
column over the two strings, a strict reader of the file, and the CIGAR read back from two rows.  No GPU, nothing of ntsynt_amd."""
import re

I, D, EQ, X = 1, 2, 7, 8
LETTER = {I: "I", D: "D", EQ: "=", X: "X"}
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
S_LINE = re.compile(r"^s (\S+) (\d+) (\d+) ([+-]) (\d+) ([ACGTN-]+)$")


def letters(seq):
    "a sequence (str, bytes or ASCII uint8 array) as the rows spell it: upper case, N for what is no base"
    if not isinstance(seq, str):
        seq = bytes(bytearray(int(v) for v in seq)).decode()
    return "".join(ch if ch in "ACGT" else "N" for ch in seq.upper())


def reverse_complement(seq):
    return "".join(COMPLEMENT[ch] for ch in reversed(letters(seq)))


def rows_from_cigar(entries, target, query_as_read):
    "(row A, row B) of one chain: target read forwards, query as read, one column at a time"
    target, query = letters(target), letters(query_as_read)
    row_a, row_b, i, j = [], [], 0, 0
    for v in entries:
        n, code = int(v) >> 4, int(v) & 15
        if code not in LETTER:
            raise ValueError(f"no CIGAR code: {code}")
        for _ in range(n):
            if code == I:
                row_a.append("-")
            else:
                row_a.append(target[i])
                i += 1
            if code == D:
                row_b.append("-")
            else:
                row_b.append(query[j])
                j += 1
    assert (i, j) == (len(target), len(query)), "the entries do not consume the two strings"
    return "".join(row_a), "".join(row_b)


def cigar_of_rows(row_a, row_b):
    """the run-length CIGAR text of two rows: a gap in row A is I, in row B is D, equal bases are =, unequal ones X; a column with an N on
    either side is X, as in the CIGARs of the alignment pass, where what is no base matches nothing; neighbouring columns of one kind
    are one run"""
    assert len(row_a) == len(row_b)
    runs = []
    for a, b in zip(row_a, row_b):
        assert (a, b) != ("-", "-"), "a column of two gaps"
        letter = "I" if a == "-" else "D" if b == "-" else "=" if a == b and a != "N" else "X"
        if runs and runs[-1][0] == letter:
            runs[-1][1] += 1
        else:
            runs.append([letter, 1])
    return "".join(f"{n}{letter}" for letter, n in runs)


def parse_maf(text):
    """the blocks of a pairwise MAF file, read strictly: the header `##maf version=1` and a blank line, then per block `a score=<n>`,
    two `s` lines of single-blank-separated fields and a blank line; rows of equal length, size = the non-gap bytes, start + size inside
    the record, the first line on `+`.  Returns dicts: score, and per line (t_ / q_) name, start, size, strand, src_size, row."""
    header = "##maf version=1\n\n"
    assert text.startswith(header) and text.endswith("\n"), "header or end of file"
    body = text[len(header):].split("\n")[:-1]
    assert len(body) % 4 == 0, "a block has four lines"
    out = []
    for at in range(0, len(body), 4):
        head, first, second, blank = body[at:at + 4]
        m = re.match(r"^a score=(\d+)$", head)
        assert m and blank == "", (at, head[:80], blank[:80])
        block = {"score": int(m.group(1))}
        for side, line in (("t", first), ("q", second)):
            s = S_LINE.match(line)
            assert s, (at, line[:120])
            name, start, size, strand, src_size, row = s.groups()
            start, size, src_size = int(start), int(size), int(src_size)
            assert size == len(row) - row.count("-") and size > 0 and start + size <= src_size, (at, name, start, size, src_size)
            block.update({f"{side}_name": name, f"{side}_start": start, f"{side}_size": size, f"{side}_strand": strand, f"{side}_src_size": src_size,
                          f"{side}_row": row})
        assert block["t_strand"] == "+" and len(block["t_row"]) == len(block["q_row"]), at
        out.append(block)
    return out

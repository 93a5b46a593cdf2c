"""Brute force for nts_cigar_build (docs/design/04_22_block_alignments.md), the definitions taken literally: the column list of every
piece, reversed where the piece says so, concatenated per chain and run-length encoded; and apply_cigar, which walks a CIGAR over two
strings.  No GPU, nothing of ntsynt_amd."""
SUB, DEL, INS = 1, 2, 3
REVERSED = 1
CODE = {"I": 1, "D": 2, "=": 7, "X": 8}                       # BAM's codes
LETTER = {v: k for k, v in CODE.items()}


class NoScript(ValueError):
    "the ops of a piece break a column rule; .piece = its index"

    def __init__(self, piece, why):
        super().__init__(f"piece {piece}: {why}")
        self.piece = piece


def piece_columns(t, n, m, ops):
    """the columns of piece t as (letter, length) runs, zero-length runs included, in path order.  ops: (seg, p, q, op, ...) tuples in
    ascending path order"""
    i = j = 0
    out = []
    for op in ops:
        seg, p, q, code = (int(v) for v in op[:4])
        if seg != t:
            raise NoScript(t, f"an op with seg {seg}")
        if code not in (SUB, DEL, INS):
            raise NoScript(t, f"op code {code}")
        g = p - i
        if g != q - j or g < 0:
            raise NoScript(t, f"op at ({p}, {q}) behind ({i}, {j})")
        out.append(("=", g))
        if code == SUB:
            if not (p < n and q < m):
                raise NoScript(t, "SUB beyond a string")
            out.append(("X", 1))
            i, j = p + 1, q + 1
        elif code == DEL:
            if not (p < n and q <= m):
                raise NoScript(t, "DEL beyond a string")
            out.append(("D", 1))
            i, j = p + 1, q
        else:
            if not (p <= n and q < m):
                raise NoScript(t, "INS beyond a string")
            out.append(("I", 1))
            i, j = p, q + 1
    if n - i != m - j or n - i < 0:
        raise NoScript(t, f"({i}, {j}) behind the last op does not reach ({n}, {m}) along the diagonal")
    out.append(("=", n - i))
    return out


def brute_cigar(pieces, ops, first, n_chains):
    """(entries, chains): entries = [len << 4 | code] of all chains one behind the other; chains = one dict of first, n_cig, eq, x, ins,
    del, len_a, len_b per chain.  pieces: (chain, n, m, flags); ops: tuples (seg, p, q, op, ...); first: n_pieces + 1 offsets.  The
    smallest piece whose ops are no script raises NoScript."""
    runs_of = [[] for _ in range(n_chains)]
    sums = [[0, 0] for _ in range(n_chains)]
    for t, piece in enumerate(pieces):
        chain, n, m, flags = (int(v) for v in piece)
        cols = piece_columns(t, n, m, ops[int(first[t]):int(first[t + 1])])
        runs_of[chain] += cols[::-1] if flags & REVERSED else cols
        sums[chain][0] += n
        sums[chain][1] += m
    entries, chains = [], []
    for c in range(n_chains):
        merged = []
        for letter, length in runs_of[c]:
            if length == 0:
                continue
            if merged and merged[-1][0] == letter:
                merged[-1][1] += length
            else:
                merged.append([letter, length])
        count = {k: sum(n for letter, n in merged if letter == k) for k in "=XID"}
        rec = {"first": len(entries), "n_cig": len(merged), "eq": count["="], "x": count["X"], "ins": count["I"],
               "del": count["D"], "len_a": count["="] + count["X"] + count["D"], "len_b": count["="] + count["X"] + count["I"]}
        assert (rec["len_a"], rec["len_b"]) == tuple(sums[c])
        chains.append(rec)
        entries += [(length << 4) | CODE[letter] for letter, length in merged]
    return entries, chains


def cigar_string(entries):
    return "".join(f"{int(e) >> 4}{LETTER[int(e) & 15]}" for e in entries)


def parse_cigar(text):
    "[(length, letter)] of an =/X/I/D CIGAR string"
    out, number = [], ""
    for ch in text:
        if ch.isdigit():
            number += ch
        else:
            assert ch in CODE and number and int(number) > 0, text[:80]
            out.append((int(number), ch))
            number = ""
    assert number == ""
    return out


def apply_cigar(target, query, cigar):
    """walks a CIGAR (a string, or entries len << 4 | code) over two strings (str, bytes or uint8 arrays): `=` on equal bases, `X` on
    unequal ones, both lengths consumed exactly, no two neighbouring runs of one kind.  Returns (eq, x, ins, del)."""
    runs = parse_cigar(cigar) if isinstance(cigar, str) else [(int(e) >> 4, LETTER[int(e) & 15]) for e in cigar]
    t = target.encode() if isinstance(target, str) else bytes(bytearray(target))
    q = query.encode() if isinstance(query, str) else bytes(bytearray(query))
    i = j = 0
    count = {k: 0 for k in "=XID"}
    last = None
    for length, letter in runs:
        assert length > 0 and letter != last, (length, letter, last)
        last = letter
        count[letter] += length
        if letter in "=X":
            assert i + length <= len(t) and j + length <= len(q), (i, j, length, letter)
            if letter == "=":
                assert t[i:i + length] == q[j:j + length], (i, j, length)
            else:
                assert all(t[i + d] != q[j + d] for d in range(length)), (i, j, length)
            i, j = i + length, j + length
        elif letter == "D":
            i += length
        else:
            j += length
    assert (i, j) == (len(t), len(q)), (i, j, len(t), len(q))
    return count["="], count["X"], count["I"], count["D"]

"""Brute forces for the cs:Z: tag (docs/design/04_26_block_paf_cs.md), straight from the definition: the text of a CIGAR walked column by
column over the two strings, the query rebuilt from the text and the target, and the CIGAR read back from the text.  No GPU, nothing of
ntsynt_amd."""
import re

I, D, EQ, X = 1, 2, 7, 8
LETTER = {I: "I", D: "D", EQ: "=", X: "X"}
SUB, DEL, INS = 1, 2, 3                                      # tests/variants_brute.script's ops
TOKEN = re.compile(r":([0-9]+)|\*([acgtn])([acgtn])|-([acgtn]+)|\+([acgtn]+)")
COMPLEMENT = {"a": "t", "c": "g", "g": "c", "t": "a", "n": "n"}


def letters(seq):
    "a sequence (str, bytes or ASCII uint8 array) as the tag spells it: lower case, n for what is no base"
    if not isinstance(seq, str):
        seq = bytes(bytearray(int(v) for v in seq)).decode()
    return "".join(ch if ch in "acgt" else "n" for ch in seq.lower())


def reverse_complement(seq):
    return "".join(COMPLEMENT[ch] for ch in reversed(letters(seq)))


def cg_from_cigar(entries):
    return "".join(f"{int(v) >> 4}{LETTER[int(v) & 15]}" for v in entries)


def cs_from_cigar(entries, target, query):
    "the short cs text of one chain: target read forwards, query as read, one column at a time"
    target, query = letters(target), letters(query)
    out, i, j = [], 0, 0
    for v in entries:
        n, code = int(v) >> 4, int(v) & 15
        if code == EQ:
            out.append(f":{n}")
            i, j = i + n, j + n
        elif code == X:
            for _ in range(n):
                out.append("*" + target[i] + query[j])
                i, j = i + 1, j + 1
        elif code == D:
            out.append("-")
            for _ in range(n):
                out.append(target[i])
                i += 1
        elif code == I:
            out.append("+")
            for _ in range(n):
                out.append(query[j])
                j += 1
        else:
            raise ValueError(f"no CIGAR code: {code}")
    assert (i, j) == (len(target), len(query)), "the entries do not consume the two strings"
    return "".join(out)


def tokens(cs):
    "the text taken apart: (kind, payload) with kind one of : * - +"
    out, at = [], 0
    while at < len(cs):
        m = TOKEN.match(cs, at)
        assert m, f"no cs token at {at}: {cs[at:at + 20]!r}"
        if m.group(1) is not None:
            out.append((":", int(m.group(1))))
        elif m.group(2) is not None:
            out.append(("*", (m.group(2), m.group(3))))
        elif m.group(4) is not None:
            out.append(("-", m.group(4)))
        else:
            out.append(("+", m.group(5)))
        at = m.end()
    return out


def apply_cs(cs, target):
    "the query that the text makes of the target; every : run, - base and * target base is asserted against the target"
    target = letters(target)
    out, i = [], 0
    for kind, what in tokens(cs):
        if kind == ":":
            assert what > 0 and i + what <= len(target), "a match run beyond the target"
            out.append(target[i:i + what])
            i += what
        elif kind == "*":
            assert i < len(target) and target[i] == what[0], f"* names {what[0]} at target base {i}, which is {target[i:i + 1]}"
            out.append(what[1])
            i += 1
        elif kind == "-":
            assert target[i:i + len(what)] == what, f"- names {what} at target base {i}, which is {target[i:i + len(what)]}"
            i += len(what)
        else:
            out.append(what)
    assert i == len(target), f"the text consumes {i} of {len(target)} target bases"
    return "".join(out)


def cigar_of_cs(cs):
    "the run-length CIGAR text of a cs text: neighbouring tokens of one kind are one run"
    runs = []
    for kind, what in tokens(cs):
        letter, n = {":": "=", "*": "X", "-": "D", "+": "I"}[kind], what if kind == ":" else 1 if kind == "*" else len(what)
        if runs and runs[-1][0] == letter:
            runs[-1][1] += n
        else:
            runs.append([letter, n])
    return "".join(f"{n}{letter}" for letter, n in runs)


def entries_of_script(ops, n, m):
    "CIGAR entries (maximal runs) of tests/variants_brute.script's (op, p, q) list over strings of n and m bases"
    columns, i, j = [], 0, 0
    for op, p, q in ops:
        assert p - i == q - j >= 0
        columns += [EQ] * (p - i)
        i, j = p, q
        if op == SUB:
            columns.append(X)
            i, j = i + 1, j + 1
        elif op == DEL:
            columns.append(D)
            i += 1
        else:
            columns.append(I)
            j += 1
    assert n - i == m - j >= 0
    columns += [EQ] * (n - i)
    out = []
    for code in columns:
        if out and out[-1][1] == code:
            out[-1][0] += 1
        else:
            out.append([1, code])
    return [length << 4 | code for length, code in out]

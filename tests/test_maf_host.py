"""assess.maf_block, assess.maf_table and assess.maf_rows_host (docs/design/04_29_block_maf.md) on hand-made chains, byte for byte; the
strict reader of tests/maf_brute.py on what they write; and the brute helpers against tests/cs_brute.py on random CIGARs.  No GPU."""
import numpy as np
import pytest

from ntsynt_amd import assess
from tests import cs_brute as CS
from tests import maf_brute as MB

I, D, EQ, X = 1, 2, 7, 8

#        name_a, rec_len_a, tstart, len_a, name_b, rec_len_b, qstart, qend, minus, eq, x, row_a, row_b
PLUS = ("g0.fa.chr1", 1000, 10, 9, "g1.fa.chr2", 900, 20, 28, False, 6, 1, "ACGTAC-GTA", "ACGAACTG--")
MINUS = ("g0.fa.chr1", 1000, 100, 6, "g2.fa.chrX", 500, 40, 47, True, 5, 1, "ACG-TAC", "ACGTTAG")
ALL_EQ = ("g0.fa.chr3", 12, 0, 12, "g1.fa.chr3", 12, 0, 12, False, 12, 0, "ACGTACGTACGT", "ACGTACGTACGT")
NO_MATCH = ("g0.fa.chr1", 1000, 300, 3, "g1.fa.chr2", 900, 400, 402, True, 0, 0, "ACG--", "---TT")


def test_maf_block_gives_the_exact_lines():
    assert assess.maf_block(*PLUS[:10], *PLUS[11:]) == ("a score=6\n"
                                                        "s g0.fa.chr1 10 9 + 1000 ACGTAC-GTA\n"
                                                        "s g1.fa.chr2 20 8 + 900 ACGAACTG--\n"
                                                        "\n")
    # a `-` line starts on the reverse strand: start_b = rec_len_b - qend = 500 - 47
    assert assess.maf_block(*MINUS[:10], *MINUS[11:]) == ("a score=5\n"
                                                          "s g0.fa.chr1 100 6 + 1000 ACG-TAC\n"
                                                          "s g2.fa.chrX 453 7 - 500 ACGTTAG\n"
                                                          "\n")
    assert assess.maf_block(*ALL_EQ[:10], *ALL_EQ[11:]) == "a score=12\ns g0.fa.chr3 0 12 + 12 ACGTACGTACGT\ns g1.fa.chr3 0 12 + 12 ACGTACGTACGT\n\n"
    assert "  " not in assess.maf_block(*PLUS[:10], *PLUS[11:]) and "\t" not in assess.maf_block(*PLUS[:10], *PLUS[11:])


def test_maf_table_gives_the_exact_file_and_leaves_out_a_chain_without_a_match_column():
    text = assess.maf_table([PLUS, NO_MATCH, MINUS, ALL_EQ])
    assert text == ("##maf version=1\n\n"
                    "a score=6\ns g0.fa.chr1 10 9 + 1000 ACGTAC-GTA\ns g1.fa.chr2 20 8 + 900 ACGAACTG--\n\n"
                    "a score=5\ns g0.fa.chr1 100 6 + 1000 ACG-TAC\ns g2.fa.chrX 453 7 - 500 ACGTTAG\n\n"
                    "a score=12\ns g0.fa.chr3 0 12 + 12 ACGTACGTACGT\ns g1.fa.chr3 0 12 + 12 ACGTACGTACGT\n\n")
    assert assess.maf_table([]) == "##maf version=1\n\n" and assess.maf_table([NO_MATCH]) == "##maf version=1\n\n"
    only_x = NO_MATCH[:9] + (0, 1) + NO_MATCH[11:]           # one mismatch column is an aligned base pair: the block is written
    assert assess.maf_table([only_x]).count("a score=0\n") == 1


def test_parse_maf_round_trips():
    parts = [PLUS, MINUS, ALL_EQ]
    blocks = MB.parse_maf(assess.maf_table(parts + [NO_MATCH]))
    assert len(blocks) == 3
    for part, b in zip(parts, blocks):
        name_a, rec_len_a, tstart, len_a, name_b, rec_len_b, qstart, qend, minus, eq, x, row_a, row_b = part
        assert (b["score"], b["t_name"], b["t_start"], b["t_size"], b["t_strand"], b["t_src_size"], b["t_row"]) == (eq, name_a, tstart, len_a, "+", rec_len_a, row_a)
        assert (b["q_name"], b["q_size"], b["q_strand"], b["q_src_size"], b["q_row"]) == (name_b, qend - qstart, "-" if minus else "+", rec_len_b, row_b)
        forward_start = b["q_src_size"] - b["q_start"] - b["q_size"] if minus else b["q_start"]     # back from the reverse strand
        assert forward_start == qstart
    for bad in ("##maf version=1\n", "##maf version=1\n\na score=1\ns a 0 1 + 5 A\n\n", assess.maf_table([PLUS]).replace(" 9 + ", " 8 + "),
                assess.maf_table([PLUS]).replace("s g0.fa.chr1 10", "s  g0.fa.chr1 10"), assess.maf_table([PLUS]).replace("ACGAACTG--", "ACGAACTG-")):
        with pytest.raises(AssertionError):
            MB.parse_maf(bad)


def random_chain(rng):
    "(entries -- not maximal runs --, target, query) that agree: = on equal bases, X on unequal ones or on an N"
    entries, target, query = [], [], []
    for _ in range(int(rng.integers(1, 30))):
        code, n = int(rng.choice([EQ, EQ, X, I, D])), int(rng.integers(1, 9))
        entries.append(n << 4 | code)
        for _ in range(n):
            a = "ACGT"[int(rng.integers(0, 4))]
            if code == EQ:
                target.append(a)
                query.append(a)
            elif code == X:
                kind = int(rng.integers(0, 8))
                b = "ACGT".replace(a, "")[int(rng.integers(0, 3))]
                target.append("N" if kind in (0, 2) else a)
                query.append("N" if kind in (1, 2) else b)   # (kind 2: N against N is a mismatch column)
            elif code == D:
                target.append("N" if rng.integers(0, 10) == 0 else a)
            else:
                query.append("N" if rng.integers(0, 10) == 0 else a)
    return entries, "".join(target), "".join(query)


def test_the_brute_helpers_agree_with_cs_brute_on_random_cigars():
    rng = np.random.default_rng(2901)
    kinds = set()
    for _ in range(300):
        entries, target, query = random_chain(rng)
        row_a, row_b = MB.rows_from_cigar(entries, target, query)
        merged = CS.cigar_of_cs(CS.cs_from_cigar(entries, target, query))
        assert MB.cigar_of_rows(row_a, row_b) == merged
        assert (row_a.replace("-", ""), row_b.replace("-", "")) == (target, query)
        assert len(row_a) == len(row_b) == sum(v >> 4 for v in entries)
        # lower case input and what is no base: the rows are upper case with N
        assert MB.rows_from_cigar(entries, target.lower().replace("n", "r"), query.lower()) == (row_a, row_b)
        host_a, host_b = assess.maf_rows_host(np.array(entries, dtype=np.uint64), np.frombuffer(target.encode(), dtype=np.uint8),
                                              np.frombuffer(query.encode(), dtype=np.uint8))
        assert (host_a.tobytes().decode(), host_b.tobytes().decode()) == (row_a, row_b)
        kinds |= set(re_letters(merged))
    assert kinds == set("=XID")
    assert MB.reverse_complement("ACGTNacgtr") == "NACGTNACGT" and MB.reverse_complement("AAC") == CS.reverse_complement("AAC").upper()
    assert MB.cigar_of_rows("NN-A", "NNA-") == "2X1I1D" and MB.cigar_of_rows("ACGT", "ACGT") == "4="
    with pytest.raises(ValueError):
        assess.maf_rows_host(np.array([3 << 4 | EQ], dtype=np.uint64), np.frombuffer(b"AC", dtype=np.uint8), np.frombuffer(b"ACG", dtype=np.uint8))


def re_letters(cigar):
    return [ch for ch in cigar if not ch.isdigit()]

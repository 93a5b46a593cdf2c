"""The cs:Z: tag on the CPU (docs/design/04_26_block_paf_cs.md): tests/cs_brute.py against hand-written cases and, on random strings, against
the canonical scripts of tests/variants_brute.py (the text rebuilds the query and gives back the CIGAR); assess.alignment_spans against
paf_row's coordinates on both strands; paf_row's tag order with and without the tag.  No GPU."""
from collections import namedtuple

import numpy as np
import pytest

from ntsynt_amd import assess
from tests import cs_brute as CS
from tests import lift_brute as LB
from tests import variants_brute as V


def test_hand_written_texts():
    entries = LB.parse_cigar("3=1X2D2=3I1=")
    target, query = "ACGTTTGAC", "ACGAGACCCC"                  # ACG T->A, TT deleted, GA, CCC inserted, C
    cs = CS.cs_from_cigar(entries, target, query)
    assert cs == ":3*ta-tt:2+ccc:1"
    assert CS.cg_from_cigar(entries) == "3=1X2D2=3I1="
    assert CS.apply_cs(cs, target) == query.lower()
    assert CS.cigar_of_cs(cs) == "3=1X2D2=3I1="
    assert CS.tokens(cs) == [(":", 3), ("*", ("t", "a")), ("-", "tt"), (":", 2), ("+", "ccc"), (":", 1)]
    # entries that are no maximal runs: the text keeps them apart, the CIGAR read back merges them
    split = LB.parse_cigar("2=1=1X1D1D2=1I2I1=")
    cs = CS.cs_from_cigar(split, target, query)
    assert cs == ":2:1*ta-t-t:2+c+cc:1" and CS.cigar_of_cs(cs) == "3=1X2D2=3I1=" and CS.apply_cs(cs, target) == query.lower()
    # what is no base is n, on either side; X runs give one *tq per column
    assert CS.cs_from_cigar(LB.parse_cigar("3X1D1I"), "ANRG", "NCTN") == "*an*nc*nt-g+n"
    assert CS.cs_from_cigar([], "", "") == "" and CS.cigar_of_cs("") == "" and CS.apply_cs("", "") == ""
    assert CS.reverse_complement("AACGN") == "ncgtt" and CS.letters(np.frombuffer(b"acGTx", dtype=np.uint8)) == "acgtn"


def test_apply_cs_asserts_against_the_target():
    for cs, target in ((":4", "ACG"), (":2", "ACG"), ("*ca:2", "ACG"), ("-cc:1", "ACG"), (":3-a", "ACG")):
        with pytest.raises(AssertionError):
            CS.apply_cs(cs, target)
    with pytest.raises(AssertionError):
        CS.tokens(":3=2")
    with pytest.raises(AssertionError):
        CS.cs_from_cigar(LB.parse_cigar("3="), "ACG", "AC")


def mutate(rng, a, edits):
    b = list(a)
    for _ in range(edits):
        at, kind = int(rng.integers(0, len(b) + 1)), int(rng.integers(0, 3))
        if kind == 0 and at < len(b):
            b[at] = int(rng.choice([c for c in b"ACGT" if c != b[at]]))
        elif kind == 1 and at < len(b):
            del b[at:at + int(rng.integers(1, 4))]
        else:
            b[at:at] = rng.choice(list(b"ACGT"), int(rng.integers(1, 4))).tolist()
    return np.array(b, dtype=np.uint8)


def test_round_trip_on_random_scripts():
    rng = np.random.default_rng(2600)
    kinds = set()
    for trial in range(60):
        a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(rng.integers(1, 90)))]
        b = mutate(rng, a, int(rng.integers(0, 7)))
        ops = V.script(a, b)
        entries = CS.entries_of_script(ops, a.size, b.size)
        cs = CS.cs_from_cigar(entries, a, b)
        assert CS.apply_cs(cs, a) == CS.letters(b), trial
        assert CS.cigar_of_cs(cs) == CS.cg_from_cigar(entries), trial
        assert cs.count("*") + sum(len(w) for k, w in CS.tokens(cs) if k in "-+") == len(ops), trial
        kinds |= {k for k, _ in CS.tokens(cs)}
        back = CS.cs_from_cigar(entries, a, CS.reverse_complement(CS.reverse_complement(b)))   # (the complement twice is the string)
        assert back == cs
    assert kinds == set(":*-+")


Round = namedtuple("Round", ["iv_a", "iv_b", "flip", "lines"])
Line = namedtuple("Line", ["contig", "block_id", "genome"])


def test_alignment_spans_are_paf_rows_coordinates_on_both_strands():
    from ntsynt_amd.device import CIG_B_BACKWARDS, CIG_SPAN_DTYPE
    iv_a = np.array([(0, 100, 900), (1, 50, 450), (0, 1000, 1400)], dtype=np.uint64)
    iv_b = np.array([(2, 300, 1200), (0, 0, 380), (1, 70, 500)], dtype=np.uint64)
    flip = np.array([0, 1, 1], dtype=np.uint8)
    lines = [(10, 11, 0), (12, 13, 1), (14, 15, 2)]          # (line a, line b, index of a's interval)
    chains = {"line": np.array([0, 0, 1, 2, 2]), "ch": np.array([0, 1, 0, 0, 1]), "x0": np.array([5, 400, -20, 0, 200]),
              "x1": np.array([300, 790, 390, 150, 400]), "y0": np.array([7, 410, -30, 0, 210]), "y1": np.array([310, 900, 380, 160, 430])}
    spans = assess.alignment_spans(Round(iv_a, iv_b, flip, lines), chains)
    assert spans.dtype == CIG_SPAN_DTYPE and spans.shape == (5,) and not spans["pad"].any()
    record = {"eq": 1, "x": 0, "ins": 0, "del": 0}
    for c in range(5):
        q = int(chains["line"][c])
        i = lines[q][2]
        row = assess.paf_row(Line("ta", 1, "ga"), Line("qb", 1, "gb"), 5000, 6000, iv_a[i], iv_b[i], bool(flip[i]), chains["ch"][c],
                             [chains[f][c] for f in ("x0", "x1", "y0", "y1")], record, "1=").split("\t")
        q_from, q_to, sign, t_from = int(row[2]), int(row[3]), row[4], int(row[7])
        assert int(spans["pos_a"][c]) == t_from and (int(spans["rec_a"][c]), int(spans["rec_b"][c])) == (int(iv_a[i][0]), int(iv_b[i][0]))
        if sign == "+":
            assert int(spans["flags"][c]) == 0 and int(spans["pos_b"][c]) == q_from
        else:                                                 # the first base as read is the last one of the forward interval
            assert int(spans["flags"][c]) == CIG_B_BACKWARDS and int(spans["pos_b"][c]) == q_to - 1
        assert q_to - q_from == int(chains["y1"][c] - chains["y0"][c])
    empty = assess.alignment_spans(Round(iv_a, iv_b, flip, lines), {f: np.zeros(0, dtype=np.int64) for f in chains})
    assert empty.shape == (0,) and empty.dtype == CIG_SPAN_DTYPE
    with pytest.raises(ValueError):
        assess.alignment_spans(Round(iv_a, iv_b, flip, lines), dict(chains, x0=np.array([5, 400, -60, 0, 200])))


def test_paf_row_appends_the_tag_behind_cg():
    assert assess.PAF_TAGS_CS == assess.PAF_TAGS + ("cs:Z:",) and assess.PAF_TAGS[-1] == "cg:Z:"
    args = (Line("ta", 7, "ga"), Line("qb", 7, "gb"), 5000, 6000, (0, 100, 900), (2, 300, 1200), False, 0, (5, 9, 7, 10), {"eq": 3, "x": 1, "ins": 0, "del": 0})
    plain = assess.paf_row(*args, "3=1X")
    with_cs = assess.paf_row(*args, "3=1X", cs=":3*ac")
    assert with_cs == plain + "\tcs:Z::3*ac" and assess.paf_row(*args, "3=1X", None) == plain
    assert [f[:5] for f in with_cs.split("\t")[12:]] == list(assess.PAF_TAGS_CS)
    assert [f[:5] for f in plain.split("\t")[12:]] == list(assess.PAF_TAGS)
    assert assess.paf_row(*args, [3 << 4 | 7, 1 << 4 | 8], cs="").endswith("cg:Z:3=1X\tcs:Z:")

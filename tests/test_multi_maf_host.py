"""The pure host functions of the block multi-MAF (ntsynt_amd/assess.py; docs/design/04_30_block_maf_multi.md) against
tests/multi_maf_brute.py on hand-made chains and rows: core trimming, cut points and covering sets, col0, the `s` lines for `+` and `-`,
rows of `-` alone, sub-blocks with fewer than two rows, and the table.  No GPU."""
import numpy as np
import pytest

from tests import multi_maf_brute as MM
from tests.lift_brute import parse_cigar

I, D, P, EQ, X = 1, 2, 6, 7, 8


def records_of(lists):
    from ntsynt_amd.device import CHAIN_DTYPE
    recs = np.zeros(len(lists), dtype=CHAIN_DTYPE)
    at = 0
    for c, entries in enumerate(lists):
        recs[c]["first"], recs[c]["n_cig"], recs[c]["len_a"], recs[c]["len_b"] = at, len(entries), MM.len_a(entries), MM.len_b(entries)
        at += len(entries)
    return recs


@pytest.mark.parametrize("back", [False, True])
def test_core_trimming(back):
    from ntsynt_amd.assess import chain_cores
    from ntsynt_amd.device import CIG_B_BACKWARDS, CIG_SPAN_DTYPE
    texts = ["2I3D4=5=", "6=1X2D3I", "1I2D3=1I2X3D1I", "4=", "3I2D", "", "1D1X1I", "2=1I1D3="]
    lists = [parse_cigar(t) for t in texts]
    cigar = np.array([v for e in lists for v in e], dtype=np.uint64)
    spans = np.zeros(len(lists), dtype=CIG_SPAN_DTYPE)
    spans["pos_a"], spans["pos_b"], spans["flags"] = 100, 1000, CIG_B_BACKWARDS if back else 0
    first, n_cig, len_a, len_b, pos_a, pos_b = chain_cores(cigar, records_of(lists), spans)
    for c, entries in enumerate(lists):
        want, cut_a, cut_b = MM.core(entries)
        if want is None:
            assert n_cig[c] == 0, texts[c]
            continue
        assert cigar[first[c]:first[c] + n_cig[c]].tolist() == want, texts[c]
        assert (len_a[c], len_b[c]) == (MM.len_a(want), MM.len_b(want))
        assert (pos_a[c], pos_b[c]) == (100 + cut_a, 1000 - cut_b if back else 1000 + cut_b), texts[c]
    assert [int(n) for n in n_cig] == [2, 2, 3, 1, 0, 0, 1, 4]              # `ID==` gives `==`, `=X DI` gives `=X`


def group_case():
    """one group over reference bases 10 .. 40 of a reference of 100 bases: row 1 = two chains [10, 25) and [30, 40), row 2 = one chain
    [15, 35) on `-`, row 3 = one chain [20, 25) whose query row is all `-` (a D alone would be no core, so: made by hand);
    sites: slot 20 of width 2 (row 1's I) and slot 32 of width 1 (row 2's)"""
    ref = "".join("ACGT"[(7 * i) % 4] for i in range(100))
    sites = {20: 2, 32: 1}

    def rows(t0, t1, own):
        a, b = [], []
        for p in range(t0, t1):
            if p in sites:
                a.append("-" * sites[p])
                b.append(own.get(p, "").ljust(sites[p], "-"))
            a.append(ref[p])
            b.append(own.get(("d", p), ref[p]))
        return "".join(a), "".join(b)
    chains = []
    for row, t0, t1, name, src, minus, start, own in ((1, 10, 25, "q1.c", 500, False, 110, {20: "TT"}), (1, 30, 40, "q1.c", 500, False, 140, {}),
                                                      (2, 15, 35, "q2.c", 300, True, 50, {32: "G", ("d", 16): "-", ("d", 17): "-"}),
                                                      (3, 20, 25, "q3.c", 200, False, 0, {("d", p): "-" for p in range(20, 25)})):
        row_a, row_b = rows(t0, t1, own)
        chains.append({"row": row, "t0": t0, "t1": t1, "name": name, "src_size": src, "minus": minus, "start": start, "row_a": row_a, "row_b": row_b})
    return ref, sites, chains


def as_tuples(chains):
    return [(c["row"], c["t0"], c["t1"], c["name"], c["src_size"], c["minus"], c["start"], c["row_a"], c["row_b"]) for c in chains]


def test_col0_cut_points_and_covering_sets():
    from ntsynt_amd.assess import multi_maf_col0
    _, sites, chains = group_case()
    pos, w = sorted(sites), [sites[p] for p in sorted(sites)]
    for p in (10, 19, 20, 21, 32, 33, 40):
        assert int(multi_maf_col0(10, pos, w, p)) == MM.col0(10, sites, p)
    assert MM.col0(10, sites, 20) == 10 and MM.col0(10, sites, 21) == 13 and MM.col0(10, sites, 40) == 33
    spans = [(c["t0"], c["t1"]) for c in chains]
    assert MM.cuts_of(spans) == [10, 15, 20, 25, 30, 35, 40]
    assert [MM.covering(spans, a, b) for a, b in zip(MM.cuts_of(spans)[:-1], MM.cuts_of(spans)[1:])] == [[0], [0, 2], [0, 2, 3], [2], [1, 2], [1]]


def test_the_table_equals_the_brute_force_and_its_s_lines():
    from ntsynt_amd.assess import multi_maf_parts, multi_maf_table
    ref, sites, chains = group_case()
    pos, w = sorted(sites), [sites[p] for p in sorted(sites)]
    parts = multi_maf_parts("r.c", 100, as_tuples(chains), pos, w)
    text = multi_maf_table(parts)
    assert text == MM.table([("r.c", 100, chains, sites)])
    blocks = MM.parse(text)
    # [10, 15) has row 1 alone below the reference -- two rows; [25, 30) has row 2 alone; row 3 is all `-` and is left out everywhere
    assert [[r[0] for r in b] for b in blocks] == [["r.c", "q1.c"], ["r.c", "q1.c", "q2.c"], ["r.c", "q1.c", "q2.c"], ["r.c", "q2.c"], ["r.c", "q1.c", "q2.c"],
                                                   ["r.c", "q1.c"]]
    assert [b[0][1:3] for b in blocks] == [(10, 5), (15, 5), (20, 5), (25, 5), (30, 5), (35, 5)]
    assert blocks[2][0][5] == "--" + ref[20:25] and blocks[2][1][5] == "TT" + ref[20:25] and blocks[2][2][5] == "--" + ref[20:25]
    assert [b[1][1] for b in blocks if b[1][0] == "q1.c"] == [110, 115, 120, 140, 145]      # + rows: the running base count (TT counted in the third)
    assert blocks[3][1][1:4] == (50 + 3 + 5, 5, "-") and blocks[1][2][1:4] == (50, 3, "-")  # the `-` row counts on from its start; 2 bases deleted
    assert blocks[4][2][5] == ref[30:32] + "G" + ref[32:35] and blocks[4][1][5] == ref[30:32] + "-" + ref[32:35]
    assert multi_maf_table([]) == MM.MAF_HEADER


def test_a_sub_block_with_the_reference_alone_is_skipped_and_disagreement_is_an_error():
    from ntsynt_amd.assess import multi_maf_parts, multi_maf_table
    ref, sites, chains = group_case()
    pos, w = sorted(sites), [sites[p] for p in sorted(sites)]
    only = [chains[3]]                                        # the chain whose query row is all `-`: no sub-block at all
    assert multi_maf_parts("r.c", 100, as_tuples(only), pos, w) == [] and MM.table([("r.c", 100, only, sites)]) == MM.MAF_HEADER
    pair = [chains[0], chains[3]]                             # [10, 20): row 1; [20, 25): row 1 (row 3 dropped)
    assert multi_maf_table(multi_maf_parts("r.c", 100, as_tuples(pair), pos, w)) == MM.table([("r.c", 100, pair, sites)])
    bad = dict(chains[2], row_a=chains[2]["row_a"].replace("A", "C", 1))
    with pytest.raises(RuntimeError, match="disagree"):
        multi_maf_parts("r.c", 100, as_tuples([chains[0], bad]), pos, w)
    with pytest.raises(ValueError, match="overlap"):
        multi_maf_parts("r.c", 100, as_tuples([chains[0], dict(chains[1], t0=24)]), pos, w)


def test_unpadded_host_gives_the_core_back():
    from ntsynt_amd.assess import padded_rows_host, unpadded_host
    chains = [(0, 10, parse_cigar("10=2I10=")), (0, 10, parse_cigar("5=10D5=")), (0, 5, parse_cigar("15X5="))]
    padded, first = MM.pad_all(chains, 1)[:2]
    for c, (_, _, entries) in enumerate(chains):
        mine = padded[first[c]:first[c + 1]]
        assert unpadded_host(np.array(mine, dtype=np.uint64)).tolist() == entries
        target, query = "ACGT" * 5, "TGCA" * 6
        la, lb = MM.len_a(entries), MM.len_b(entries)
        t, q = np.frombuffer(target[:la].encode(), dtype=np.uint8), np.frombuffer(query[:lb].encode(), dtype=np.uint8)
        assert padded_rows_host(mine, t, q) == MM.padded_rows(mine, target[:la], query[:lb])

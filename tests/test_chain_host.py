"""The host side of the chain file (docs/design/04_28_block_chain.md) without a device: tests/chain_brute.py against hand-worked pairs,
assess.chain_header against a hand-worked `-` pair, parse_chain rejecting each malformation, and assess.chain_links against the links
_Lifter made before the helper was factored out of it, on a fabricated round of the alignment pass (fabricated_round, which
tests/test_gpu_block_chain.py imports)."""
from types import SimpleNamespace

import numpy as np
import pytest

from ntsynt_amd import assess
from tests import chain_brute as CB
from tests.test_gpu_cigar_lift import arrays

# per pair: (flipped, [(chain, open A bases in front of it, open B bases in front of it)]); the first chain's numbers are its oriented
# offsets inside the two intervals and may be negative (a flank that leaves the interval)
ROUND_PAIRS = ((False, [("5=1X3I2D4=", 4, 2)]),
               (True, [("4=2I", -3, 3), ("3D2I6=", 0, 0), ("2=", 40, 0)]),
               (False, [("2I3D", 0, 0), ("1D", 1, 0)]),                                   # no match column: no liftover chain
               (True, [("3=2D", 5, -2), ("4I2=", 5, 7), ("2I", 1, 1), ("3=", 2, 0)]),
               (False, [("1=", 0, 0), ("10=", 0, 0), ("1X2I", 0, 0), ("7=", 0, 0)]))


def fabricated_round(spec=ROUND_PAIRS, seed=3):
    """(blocks, a): block lines and an _AlignmentRound as assess._alignment_rounds yields them, fabricated in NumPy -- pair q is lines
    (2 q, 2 q + 1) of block q, target record `t<q>` of 1 000 bases with its interval at 100 .. 900, query record `q<q>` of 2 000 bases
    with its interval at 300 .. 1 500; the chain records in a random order, one chain without entries among them"""
    rng = np.random.default_rng(seed)
    flat = [(q, ch, c) for q, (_, pair) in enumerate(spec) for ch, (c, _, _) in enumerate(pair)] + [(1, 9, [])]
    order = rng.permutation(len(flat))
    cigar, records, _ = arrays([flat[i][2] for i in order.tolist()])
    chains = {f: np.zeros(len(flat), dtype=np.int64) for f in ("line", "ch", "x0", "x1", "y0", "y1")}
    at = {}
    for q, (_, pair) in enumerate(spec):
        a = b = 0
        for ch, (_, da, db) in enumerate(pair):
            at[(q, ch)] = (a + da, b + db)
            c = int(np.flatnonzero(order == [i for i, f in enumerate(flat) if f[:2] == (q, ch)][0])[0])
            a, b = a + da + int(records[c]["len_a"]), b + db + int(records[c]["len_b"])
    at[(1, 9)] = (500, 500)
    for c, i in enumerate(order.tolist()):
        q, ch, _ = flat[i]
        x0, y0 = at[(q, ch)]
        chains["line"][c], chains["ch"][c] = q, ch
        chains["x0"][c], chains["x1"][c], chains["y0"][c], chains["y1"][c] = x0, x0 + int(records[c]["len_a"]), y0, y0 + int(records[c]["len_b"])
    n = len(spec)
    blocks = [SimpleNamespace(block_id=q, genome="A.fa" if side == 0 else "B.fa", contig=f"{'tq'[side]}{q}", strand="+" if side == 0 or not spec[q][0] else "-")
              for q in range(n) for side in (0, 1)]
    iv_a = np.array([(q, 100, 900) for q in range(n)], dtype=np.int64)
    iv_b = np.array([(q, 300, 1500) for q in range(n)], dtype=np.int64)
    r = SimpleNamespace(lines=[(2 * q, 2 * q + 1, q) for q in range(n)], iv_a=iv_a, iv_b=iv_b, flip=np.array([int(f) for f, _ in spec], dtype=np.uint32),
                        g_a=SimpleNamespace(rec_len=np.full(n, 1000, dtype=np.uint64)), g_b=SimpleNamespace(rec_len=np.full(n, 2000, dtype=np.uint64)),
                        name_a="A.fa", name_b="B.fa")
    return blocks, assess._AlignmentRound(r, None, None, None, chains, cigar, records)


def test_the_brute_force_against_hand_worked_pairs():
    cigar, chains, _ = arrays(["3=2D", "4I2=", "2I3D4=1X2D1I", "2I"])
    links = np.array([(0, 0, 10, 20), (1, 0, 20, 30), (2, 0, 0, 0), (3, 0, 7, 7)], dtype=[("chain", "u4"), ("reserved", "u4"), ("a0", "u8"), ("b0", "u8")])
    pairs, blocks = CB.brute_blocks(cigar, chains, links, [0, 2, 3, 4, 4])
    # pair 0: `3=2D` at A 10 .. 15, B 20 .. 23; an open stretch of 5 and 7; `4I2=` at A 20 .. 22, B 30 .. 36: ONE gap of 2 + 5 and 7 + 4
    assert pairs[0] == (10, 22, 20, 36, 5, 0, 0, 2) and blocks[:2] == [(3, 7, 11), (2, 0, 0)]
    # pair 1: the leading 2I3D and the trailing 2D1I are outside the span; = next to X is one block
    assert pairs[1] == (3, 8, 2, 7, 4, 1, 2, 1) and blocks[2:] == [(5, 0, 0)]
    assert pairs[2] == (0,) * 8 and pairs[3] == (0,) * 8      # gaps only; no link
    assert CB.identities_hold(pairs, blocks)
    assert CB.brute_text(pairs, blocks) == (b"3\t7\t11\n2\n5\n", [0, 9, 11, 11, 11])
    assert not CB.identities_hold([(0, 4, 0, 3, 3, 0, 0, 1)], [(3, 0, 0)])


def test_the_header_of_a_minus_pair_by_hand():
    """target t1 of 1 000 bases, interval 100 .. 900; query q1 of 2 000 bases, interval 300 .. 1 500, reversed.  The liftover chain
    covers oriented offsets x 10 .. 60 and y 20 .. 75 (link offsets 13 .. 63 and 20 .. 75 with base (-3, 0)).  paf_row's forward query
    interval is [1500 - 75, 1500 - 20) = [1425, 1480); on the reverse strand of a sequence of 2 000 bases that is
    [2000 - 1480, 2000 - 1425) = [520, 575)"""
    ra, rb = SimpleNamespace(contig="t1", genome="A.fa", block_id=1), SimpleNamespace(contig="q1", genome="B.fa", block_id=1)
    record = {"a0": 13, "a1": 63, "b0": 20, "b1": 75, "eq": 44}
    assert assess.chain_header(ra, rb, 1000, 2000, (1, 100, 900), (1, 300, 1500), True, record, (-3, 0), 7) == "chain 44 t1 1000 + 110 160 q1 2000 - 520 575 7"
    assert assess.chain_header(ra, rb, 1000, 2000, (1, 100, 900), (1, 300, 1500), False, record, (-3, 0), 1) == "chain 44 t1 1000 + 110 160 q1 2000 + 320 375 1"
    row = assess.paf_row(ra, rb, 1000, 2000, (1, 100, 900), (1, 300, 1500), True, 0, (10, 60, 20, 75), {"eq": 44, "x": 6, "ins": 5, "del": 0}, "50=5I")
    assert row.split("\t")[2:4] == ["1425", "1480"] and row.split("\t")[7:9] == ["110", "160"]


GOOD = "chain 5 t 100 + 10 22 q 90 - 20 36 1\n3\t7\t11\n2\n\nchain 5 t 100 + 40 45 q 90 + 0 5 2\n5\n\n"


def test_parse_chain_reads_a_good_file_and_lifts_a_base():
    chains = CB.parse_chain(GOOD)
    assert [c["id"] for c in chains] == [1, 2] and chains[0]["blocks"] == [(3, 7, 11), (2, 0, 0)] and CB.parse_chain("") == []
    assert CB.chain_blocks(chains[0]) == [(10, 20, 3), (20, 34, 2)]
    assert CB.lift_base(chains, "t", 11) == [("q", "-", 90 - 1 - 21)] and CB.lift_base(chains, "t", 21) == [("q", "-", 90 - 1 - 35)]
    assert CB.lift_base(chains, "t", 15) == [] and CB.lift_base(chains, "t", 44) == [("q", "+", 4)] and CB.lift_base(chains, "u", 11) == []


@pytest.mark.parametrize("bad", [
    GOOD.replace("chain 5 t 100 + 10 22 q 90 - 20 36 1", "chain 5 t 100 + 10 22 q 90 - 20 36"),          # 12 header fields
    GOOD.replace("chain 5 t", "chains 5 t", 1), GOOD.replace("3\t7\t11", "0\t7\t11"), GOOD.replace("3\t7\t11", "3\t0\t0"),
    GOOD.replace("2\n\n", "2\t0\t1\n\n", 1),                     # the last line is no `size` alone
    GOOD.replace("2\n\n", "2\n", 1), GOOD.replace("2\n\n", "2\n\n\n", 1), GOOD[:-1], GOOD.replace("3\t7\t11", "3\t7"), GOOD.replace("3\t7\t11", "3 7 11"),
    GOOD.replace("10 22", "10 23"), GOOD.replace("20 36", "20 35"),                                   # the span identities
    GOOD.replace("36 1\n", "36 2\n"), GOOD.replace("t 100 + 10", "t 100 - 10"), GOOD.replace("3\t7\t11", "03\t7\t11"), GOOD.replace("40 45", "40 145")])
def test_parse_chain_rejects_each_malformation(bad):
    with pytest.raises(ValueError):
        CB.parse_chain(bad)


def links_before_the_refactoring(a):
    "what _Lifter.add_round and _Lifter._join_round computed before assess.chain_links existed, copied from that version"
    from ntsynt_amd.device import LIFT_LINK_DTYPE
    chains, n_lines = a.chains, len(a.round.lines)
    line = chains["line"]
    order = np.argsort(line, kind="stable")
    line = line[order]
    x0, y0 = (chains[f][order] for f in ("x0", "y0"))
    linked = np.flatnonzero(np.asarray(a.records["n_cig"]).astype(np.int64)[order] > 0)
    linked = linked[np.lexsort((a.chains["ch"][order][linked], line[linked]))]
    of_line = line[linked]
    pair_first = np.searchsorted(of_line, np.arange(n_lines + 1)).astype(np.int64)
    has = pair_first[1:] > pair_first[:-1]
    first = np.minimum(pair_first[:-1], max(linked.size - 1, 0))
    lx0, ly0 = x0[linked], y0[linked]
    base_x = np.where(has, np.minimum(lx0[first], 0), 0) if linked.size else np.zeros(n_lines, dtype=np.int64)
    base_y = np.where(has, np.minimum(ly0[first], 0), 0) if linked.size else np.zeros(n_lines, dtype=np.int64)
    links = np.zeros(linked.size, dtype=LIFT_LINK_DTYPE)
    links["chain"], links["a0"], links["b0"] = order[linked], lx0 - base_x[of_line], ly0 - base_y[of_line]
    return links, pair_first, base_x, base_y


def test_chain_links_are_the_links_the_lifter_made():
    for seed in (3, 4, 5):
        _, a = fabricated_round(seed=seed)
        got, want = assess.chain_links(a), links_before_the_refactoring(a)
        assert all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(got, want))
        links, pair_first, base_x, base_y = got
        assert pair_first.tolist() == [0, 1, 4, 6, 10, 14] and base_x.tolist() == [0, -3, 0, 0, 0] and base_y.tolist() == [0, 0, 0, -2, 0]
        assert int(links["a0"][1]) == 0 and int(links["b0"][6]) == 0 and links["chain"].size == np.unique(links["chain"]).size
    none = assess._AlignmentRound(SimpleNamespace(lines=[]), None, None, None, {f: np.zeros(0, dtype=np.int64) for f in ("line", "ch", "x0", "x1", "y0", "y1")},
                                  np.zeros(0, dtype=np.uint64), arrays([])[1])
    links, pair_first, base_x, base_y = assess.chain_links(none)
    assert links.size == 0 and pair_first.tolist() == [0] and base_x.size == 0 and base_y.size == 0


def test_chains_from_paf_on_the_fabricated_round():
    "the expected file from the PAF rows alone: the `-` pairs on the query's reverse strand, the pair without a match column left out"
    blocks, a = fabricated_round()
    found = {}
    assess._round_paf_rows(blocks, a, found)
    paf = assess.paf_table([row for la, lb, _ in a.round.lines for row in found[(la, lb)]])
    chains = CB.parse_chain(CB.chains_from_paf(paf))
    assert [(c["tName"], c["qStrand"], c["id"]) for c in chains] == [("t0", "+", 1), ("t1", "-", 2), ("t3", "-", 3), ("t4", "+", 4)]
    # pair 1 by hand: `4=2I` at x -3, y 3; `3D2I6=` behind it; `2=` 40 A bases on.  tStart = 100 - 3; the query interval ends at 1500:
    # forward [1500 - y1, 1500 - y0), reverse strand qStart = 2000 - 1500 + 3
    assert (chains[1]["tStart"], chains[1]["tEnd"], chains[1]["qStart"], chains[1]["qEnd"]) == (97, 152, 503, 519)
    assert chains[1]["blocks"] == [(4, 3, 4), (6, 40, 0), (2, 0, 0)] and chains[1]["score"] == 12
    assert chains[3]["blocks"] == [(12, 0, 2), (7, 0, 0)]       # three closed seams: `1=`, `10=` and `1X` are one block


def test_the_switch_in_the_dry_run_and_its_refusal_under_several_ranks(tmp_path):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = []
    for j in range(2):
        paths.append(str(tmp_path / f"g{j}.fa"))
        with open(paths[-1], "w", encoding="utf-8") as fh:
            fh.write(">chr1\nACGTACGTAC\n")
    cmd = [sys.executable, os.path.join(root, "bin", "ntSynt")] + paths + ["-d", "1", "--block-chain", "--block-ends", "--identity-max-edits", "1023"]

    def run(more, **env):
        return subprocess.run(cmd + more, cwd=tmp_path, capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONPATH=root, **env))
    r = run(["--dry-run"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "block_chain (chain_blocks_scan, chain_blocks_emit, chain_text; k 21, rate 16, band 31, max_len 4096, max_edits 1023, ends_max_len " in r.stdout
    assert "block_paf" not in r.stdout and r.stdout.index("block_ends") < r.stdout.index("block_chain")
    r = run(["--dry-run", "--block-paf"])
    assert r.returncode == 0 and r.stdout.index("block_paf (") < r.stdout.index("block_chain (")
    r = run([], WORLD_SIZE="2")
    assert r.returncode != 0 and "--block-chain works from the genomes resident on one GPU" in r.stderr
    assert "ntsynt_block_stats --tsv <prefix>.synteny_blocks.tsv --fai ... --fastas ... --chain-out <prefix>.block_alignments.chain" in r.stderr
    r = subprocess.run([sys.executable, os.path.join(root, "bin", "ntSynt")] + paths + ["-d", "1", "--dry-run"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, PYTHONPATH=root))
    assert r.returncode == 0 and "block_chain" not in r.stdout

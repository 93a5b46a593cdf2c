"""The constructed inputs of tests/bloom_cases.py hold what tests/test_gpu_bloom_geometry.py relies on.  The compact k-mer numbering comes
from the records alone (tests/sketch_cases.py: Layout -- a valid k-mer has no N and lies inside one record, a run is a maximal stretch
of valid k-mers with contiguous bases), a tile is 8192 consecutive compact indices, a lane 8 of them, workgroup and turn of a tile are
t % 3 and t // 3; filter indices are O.hash_all(...) % bits.  Capacities and shapes come from the host plan (nts_bf_bin_plan).  No GPU."""
import numpy as np
import pytest

from ntsynt_amd.device import bf_bin_plan
from oracle import nts_oracle as O
from tests import bloom_cases as BC
from tests.sketch_cases import Layout

T, LANE, G = BC.TILE, BC.LANE, BC.GRID


class Tiles:
    def __init__(self, records, k):
        self.lay = lay = Layout(records, k)
        self.V = lay.n_valid
        self.n_tiles = (self.V + T - 1) // T
        self.run_of = np.repeat(np.arange(lay.run_n.size), lay.run_n)          # run of every compact index

    def runs_in(self, t):
        return np.unique(self.run_of[t * T:(t + 1) * T])

    def whole(self, t):
        "all 8192 k-mers there, in one run"
        return (t + 1) * T <= self.V and self.runs_in(t).size == 1

    def pieces(self, t):
        return self.runs_in(t).size > 1

    def apart_lanes(self, t):
        "lanes of the tile whose k-mers lie in more than one run"
        r = self.run_of[t * T:min((t + 1) * T, self.V)]
        return sum(1 for a in range(0, r.size, LANE) if r[a] != r[min(a + LANE, r.size) - 1])


@pytest.mark.parametrize("k", BC.SEAM_KS)
def test_seam_cases_hold_their_claims(k):
    cases = BC.seam_cases(k)
    records, _, filters, c = cases["seams"]
    assert filters == BC.SEAM_FILTERS and all(len(s) >= k for s in records)
    x = Tiles(records, k)
    lay = x.lay
    assert x.n_tiles == 13 and x.V % T != 0
    t = c["boundary_on_j0"]                                       # a run begins on the tile's first k-mer, in a turn behind the first
    assert t * T in lay.run_first and t // G >= 1
    assert (c["run_ends_on_tile_end"] + 1) * T - 1 in lay.run_last
    t = c["carried_run_ends_on_j0"]                               # one run from J0 of the workgroup's tile before to J0 of this one
    j = int(np.flatnonzero(lay.run_first == (t - G) * T)[0])
    assert lay.run_last[j] == t * T - 1 and t - G >= 0
    turns = set()
    for t in c["whole_between_pieces"]:                           # pieces, whole, pieces in three turns of one workgroup; both parities
        assert x.whole(t) and x.pieces(t - G) and x.pieces(t + G) and t - G >= 0
        turns.add((t // G) % 2)
    assert turns == {0, 1}
    t = c["side_overflow_then_whole"]
    assert x.apart_lanes(t) > BC.SIDE_LANES and x.whole(t + G)
    ones = lay.run_n == 1
    r = x.run_of
    assert any(np.unique(r[a:a + LANE]).size == LANE for a in range(0, x.V - LANE + 1, LANE)) == c["lane_of_eight_runs"]
    t = c["gallop_from"]                                          # the carried run moves on by at least seventy one-k-mer runs
    assert int(ones[r[t * T]:r[(t + G) * T]].sum()) >= 70 and t + G < x.n_tiles
    assert (x.n_tiles - 1) // G == c["partial_last_turn"] >= 1
    # the whole tiles of the docstring, and nothing else whole
    assert [t for t in range(x.n_tiles) if x.whole(t)] == [0, 4, 5, 6, 10, 11]

    records, _, _, c = cases["carried"]
    x = Tiles(records, k)
    assert c["carried_run"] and x.lay.run_n.max() > 4 * G * T and x.n_tiles > 4 * G

    counts = []
    for n in (1, 2, 3, 4, 5):
        records, _, _, c = cases[f"tiles{n}"]
        x = Tiles(records, k)
        assert x.n_tiles == c["n_tiles"] == n and x.V - (n - 1) * T == 1 and c["last_tile_of_one"]
        counts.append(n)
    for grid in (3, 4):
        assert {grid - 1, grid, grid + 1} <= set(counts)


def test_repeat_case_overflows_once_in_each_parity_and_an_ordinary_tile_follows():
    records, k, filters, c = BC.repeat_case()
    assert k == 24 and records[1] == BC.REPEATS[0] and records[4] == BC.REPEATS[1] and c["bypass"]
    x = Tiles(records, k)
    over = c["overflow_then_ordinary"]
    assert {(t // G) % 2 for t in over} == {0, 1}
    h0 = np.concatenate([O.hash_all(s, k)[1] for s in records])
    assert h0.size == x.V
    for nbytes in filters:
        plan = bf_bin_plan(x.V, nbytes, k)
        assert plan["log2_b2"] + BC.FINAL_SHIFT == BC.LEVEL1_SHIFT[nbytes]
        bucket = ((h0 % np.uint64(nbytes * 8)) >> np.uint64(BC.LEVEL1_SHIFT[nbytes])).astype(np.int64)
        total = np.bincount(bucket, minlength=plan["B1"])
        assert total.size == plan["B1"]
        for t in over:
            # the tiles the same workgroup took before reserved first, whatever the other workgroups do: with them alone the tile is over
            mine = np.bincount(bucket[t * T:(t + 1) * T], minlength=plan["B1"])
            before = sum(np.bincount(bucket[u * T:(u + 1) * T], minlength=plan["B1"]) for u in range(t % G, t, G))
            assert ((mine > 0) & (before + mine > plan["cap1"])).any(), (nbytes, t)
            # three tiles on: whole, one run, and no bucket it touches ever holds more than cap1 -- in whatever order the tiles reserve
            nxt = np.unique(bucket[(t + G) * T:(t + G + 1) * T])
            assert x.whole(t + G) and total[nxt].max() <= plan["cap1"], (nbytes, t, int(total[nxt].max()), plan["cap1"])


def test_the_recorded_kmers_are_what_the_search_finds():
    "tests/golden/bloom_searched_kmers.json against the walk over the fixed-seed sequence that made it"
    assert BC.searched_kmers() == BC.search_kmers()


@pytest.mark.parametrize("nbytes", list(BC.GEOMETRY))
def test_geometry_cases_hold_their_claims(nbytes):
    (records, k, nb, c), (second, relative) = BC.geometry_case(nbytes)
    assert nb == nbytes
    h0 = np.concatenate([O.hash_all(s, k)[1] for s in records])
    assert 290000 < h0.size < 320000
    idx = h0 % np.uint64(nbytes * 8)
    p = bf_bin_plan(h0.size, nbytes, k)
    shape = {32 * BC.MIB: (512, 0, 512), 32 * BC.MIB + 8: (513, 1, 257), 32 * BC.MIB + 13: (513, 1, 257), 32 * BC.MIB + 11: (513, 1, 257),
             64 * BC.MIB: (1024, 1, 512), 64 * BC.MIB + 8: (1025, 2, 257), 1025 * 65536 - 8: (1025, 2, 257), 3 * BC.MIB + 12: (49, 0, 49),
             (1 << 29) + 8: (8193, 5, 257)}[nbytes]
    assert (p["F"], p["log2_b2"], p["B1"]) == shape, c["shape"]
    words_in_last_bucket = (nbytes + 3) // 4 - (p["F"] - 1) * (1 << (BC.FINAL_SHIFT - 5))
    if nbytes in (32 * BC.MIB + 11, 3 * BC.MIB + 12):
        assert words_in_last_bucket == 3                           # k_bin3's scalar tails: n_words % 4 != 0
    if nbytes == 32 * BC.MIB + 13:
        assert words_in_last_bucket == 4 and nbytes % 4 == 1      # (four words, the last of them one byte: no scalar tail at this size)
    if nbytes == (1 << 29) + 8:
        assert nbytes * 8 > 1 << 32                               # FastMod form 2
    for what in ("last_word", "last_bucket"):
        if what in c:
            lo, hi = BC.target_range(nbytes, what)
            assert hi == nbytes * 8 and int(((idx >= np.uint64(lo)) & (idx < np.uint64(hi))).sum()) >= c[what] == BC.MIN_COUNT[what]
            h_rel = np.concatenate([O.hash_all(s, k)[1] for s in relative]) % np.uint64(nbytes * 8)
            assert int((h_rel >= np.uint64(lo)).sum()) >= c[what]                      # (the AND keeps bits there)
    assert sum(what in c for what in ("last_word", "last_bucket")) == (BC.GEOMETRY[nbytes][1] is not None)
    assert p["n_final"] - p["F"] == {513: 1, 1025: 3, 8193: 31}.get(p["F"], 0)          # final buckets behind the filter's end


# ---- the inputs of tests/test_gpu_bloom_large.py ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BC.SECOND_TRIP))
def test_second_trip_cases_fill_a_final_bucket_past_one_round_of_k_bin3(name):
    """every genome of the case -- the first (store-only), the second (read-and-OR) and the relative (the AND finishes) -- fills a final
    bucket past one trip of k_bin3's load loop; without the repeats nothing is clamped, with them (the first genome and its relative)
    a level-1 bucket overflows cap1 > 16384"""
    (records, k, nbytes, c), (second, relative) = BC.second_trip_case(name)
    assert (nbytes, k) == (BC.SECOND_TRIP[name][0], BC.SECOND_TRIP_K)
    shape = {"one_bucket": (1, 0, 1), "two_buckets": (2, 0, 2), "two_buckets_over": (2, 0, 2), "packed": (513, 1, 257)}[name]
    for genome, over in ((records, c["overflow"]), (second, False), (relative, c["overflow"])):
        h0 = BC.hashes(genome, k)
        idx = h0 % np.uint64(nbytes * 8)
        p = bf_bin_plan(h0.size, nbytes, k)
        assert (p["F"], p["log2_b2"], p["B1"]) == shape and p["idx32"] == 1, c["shape"]
        final = np.bincount((idx >> np.uint64(BC.FINAL_SHIFT)).astype(np.int64), minlength=p["n_final"])
        level1 = np.bincount((idx >> np.uint64(BC.FINAL_SHIFT + p["log2_b2"])).astype(np.int64), minlength=p["B1"])
        assert final.size == p["n_final"] and level1.size == p["B1"]
        if name == "packed":
            # a second trip: more than 8192 words, i.e. more than 3 * 8192 residues whatever the partial words (here: every whole bucket)
            assert p["cap2"] > BC.BIN3_TRIP_WORDS and final[:p["F"] - 1].min() > 3 * BC.BIN3_TRIP_WORDS
            partial_words = (h0.size // p["B1"] + 1) // T + 2          # one partly filled word per tile of the level-1 bucket
            assert final.max() <= 3 * (p["cap2"] - partial_words) and level1.max() <= p["cap1"]          # nothing clamped
        elif over:
            assert BC.REPEATS[0] in genome and BC.REPEATS[1] in genome
            assert p["cap1"] > BC.BIN3_TRIP_RESIDUES and level1.max() > p["cap1"]                       # n = cap1, the rest set directly
            assert level1.min() > BC.BIN3_TRIP_RESIDUES
        else:
            assert 26400 < p["cap1"] < 26700 and level1.max() <= p["cap1"]                              # 1.125 * mean1 + 4096: unclamped
            assert final[:p["F"]].min() > BC.BIN3_TRIP_RESIDUES and final.max() < 2 * BC.BIN3_TRIP_RESIDUES   # two trips, the second partial
    assert not any(rep in second for rep in BC.REPEATS)


LARGE_PLANS = {        # nbytes -> (F, log2_b2, B2, B1, n_final)
    (1 << 30) + 8: (16385, 6, 64, 257, 16448),
    (1 << 31) + 8: (32769, 7, 128, 257, 32896),
    (1 << 32) + 8: (65537, 8, 256, 257, 65792),
    (1 << 33) + 8: (131073, 9, 512, 257, 131584),
    1 << 34: (262144, 9, 512, 512, 262144),
    16391 * 65536 + 40013: (16392, 6, 64, 257, 16448),
    131079 * 65536 + 40013: (131080, 9, 512, 257, 131584),
}


def test_large_geometries_are_what_the_table_says():
    "log2_b2 = 6 .. 9 at B1 = 257, the largest geometry, and the two sizes whose last level-1 bucket is partly real and is hit"
    assert set(BC.LARGE) == set(LARGE_PLANS) and set(BC.LARGE_PARTLY_REAL) == {16391 * 65536 + 40013, 131079 * 65536 + 40013}
    base = BC.large_base()
    sizes = [h.size for h in base["h0"]]
    assert 1_900_000 < sizes[0] < 2_100_000 and sizes[1] > 0 and sizes[2] == sizes[0]
    for nbytes, want in LARGE_PLANS.items():
        for V in sizes:
            p = bf_bin_plan(V, nbytes, BC.LARGE_K)
            assert (p["F"], p["log2_b2"], p["B2"], p["B1"], p["n_final"]) == want, BC.LARGE[nbytes]
            assert p["idx32"] == 1
    assert {LARGE_PLANS[n][1] for n in LARGE_PLANS} == {6, 7, 8, 9}
    for nbytes in BC.LARGE_PARTLY_REAL:
        F, log2_b2, B2, B1, n_final = LARGE_PLANS[nbytes]
        assert F - (B1 - 1) * B2 == 8 and n_final - F == B2 - 8 and nbytes % 65536 != 0 and nbytes % 4 != 0
        for h0 in (base["h0"][0], base["h0"][2]):                 # the first genome and its relative: the AND keeps bits there
            idx = h0 % np.uint64(nbytes * 8)
            assert int(idx.max()) < nbytes * 8
            assert int(((idx >> np.uint64(BC.FINAL_SHIFT + log2_b2)) == B1 - 1).sum()) >= 64
            assert int(((idx >> np.uint64(BC.FINAL_SHIFT)) == F - 1).sum()) >= 1
        first, both, kept = BC.sparse_reference(base["h0"], nbytes)
        assert int((kept >> np.uint64(BC.FINAL_SHIFT) == F - 1).sum()) >= 1


def test_the_sparse_reference_is_the_oracle_filter():
    """3 MiB + 12 bytes: the non-zero bytes rebuilt from the index sets (bloom_cases.sparse_reference, sparse_bytes) are O.bf_build's
    filter after insert, OR and cascade -- byte for byte, and the number of indices is its popcount"""
    from tests.helpers import to_oracle
    nbytes, k = 3 * BC.MIB + 12, BC.GEOMETRY_K
    base = BC.geometry_base()
    genomes = (base["seqs"], base["second"], base["relative"])
    og = [to_oracle([f"r{i}" for i in range(len(g))], g) for g in genomes]
    dense = [O.bf_build(og[0], k, nbytes)]
    dense.append(dense[0] | O.bf_build(og[1], k, nbytes))
    dense.append(O.bf_build(og[2], k, nbytes, prev=dense[1]))
    sparse = BC.sparse_reference([BC.hashes(g, k) for g in genomes], nbytes)
    for what, want, idx in zip(("insert", "or", "cascade"), dense, sparse):
        assert idx.dtype == np.uint64 and np.all(idx[1:] > idx[:-1]), what
        off, val = BC.sparse_bytes(idx)
        assert off.dtype == np.int64 and val.dtype == np.uint8
        assert np.array_equal(off, np.flatnonzero(want)), what
        assert np.array_equal(val, want[off]), what
        assert idx.size == O.bf_popcount(want) > 0, what
    assert sparse[0].size < sparse[1].size and 0 < sparse[2].size < sparse[0].size


@pytest.mark.parametrize("cus", [4, 256])
def test_product_case_breaks_three_turns_of_two_workgroups(cus):
    records, k, nbytes, c = BC.product_case(cus)
    x = Tiles(records, k)
    grid = 2 * cus
    assert c["grid"] == grid and x.n_tiles == c["n_tiles"] == 2 * grid + 3 and x.V % T != 0
    assert set(c["broken_tiles"]) == {b + t * grid for b in (1, 2) for t in range(3)}
    for t in range(x.n_tiles):
        assert x.pieces(t) == (t in c["broken_tiles"]), t
    p = bf_bin_plan(x.V, nbytes, k)
    assert (p["F"], p["B1"], p["log2_b2"]) == (513, 257, 1)
    if cus == 256:                                                # level-1 buckets of about four tiles: k_bin2<FULL> and its partial last tile
        assert 3 * T < x.V / p["B1"] < 5 * T and p["cap1"] > 4 * T

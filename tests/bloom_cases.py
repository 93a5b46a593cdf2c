"""Inputs for the partitioned Bloom build whose edge properties are CONSTRUCTED (tests/test_gpu_bloom_geometry.py; checked on the CPU by
tests/test_bloom_cases_host.py): genomes whose runs of valid k-mers begin, end and pile up on the seams of k_bin1's tiles and on the
turns of its persistent workgroups, and k-mers searched with the oracle's hash so that they land in a chosen stretch of a filter.
Plain numpy and the oracle; never the library under test.

k_bin1 (ntsynt_amd/csrc/nts_bloom_bin.inc) cuts the compact k-mer index into tiles of TILE = 8192, a lane takes LANE = 8 of them, and a
grid of G workgroups gives tile t to workgroup t % G in its turn t // G.  The seam cases state their claims for G = GRID = 3
(NTS_BIN1_GRID=3 on the experiments build).  A case is (records, k, nbytes, claims): nbytes one byte count or a tuple of them."""
import json
import os

import numpy as np

from oracle import nts_oracle as O

TILE, LANE, GRID, SIDE_LANES = 8192, 8, 3, 48
FINAL_SHIFT = 19
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
SEAM_FILTERS = (3 << 20, (32 << 20) + 8)                 # one partition level (48 buckets); two (F = 513: B2 = 2, B1 = 257)
LEVEL1_SHIFT = {3 << 20: 19, (32 << 20) + 8: 20}         # idx >> this = the level-1 bucket (the host test holds it against the plan)
SEAM_KS = (24, 25, 64, 65, 128)
REPEATS = (b"A" * 300000, b"ACGTTGCA" * 40000)


def bases(rng, n):
    return ACGT[rng.integers(0, 4, size=int(n))].tobytes()


def indices(seq, k, nbytes):
    "filter index of every valid k-mer of a record"
    return O.hash_all(seq, k)[1] % np.uint64(nbytes * 8)


class Runs:
    "a genome as a list of run lengths in k-mers: every run a record of its own, n + k - 1 random bases"

    def __init__(self):
        self.n, self.pos = [], 0

    def run(self, n):
        assert n >= 1
        self.n.append(int(n))
        self.pos += int(n)

    def ones(self, count):
        for _ in range(count):
            self.run(1)

    def to(self, target):
        self.run(target - self.pos)

    def records(self, rng, k):
        return [bases(rng, n + k - 1) for n in self.n]


# ---- the seam cases ---------------------------------------------------------------------------------------------------------------------
def seam_runs():
    """Thirteen tiles, the last one partial.  Workgroup 0 of three takes tiles 0 3 6 9 12, workgroup 1 tiles 1 4 7 10, workgroup 2 tiles
    2 5 8 11.  Whole single-run tiles: 0, 4, 5, 6, 10, 11; in pieces: 1, 2, 3, 7, 8, 9, 12."""
    T, r = TILE, Runs()
    r.to(T + 500)                     # tile 0 whole
    r.ones(80)                        # tile 1: eighty one-k-mer runs (the galloping search of workgroup 1's next turn) ...
    r.run(3000)
    r.ones(16)                        # ... and sixteen more in a row: some lane's eight k-mers are eight runs
    r.to(2 * T + 100)
    r.run(1000)                       # tile 2 in pieces (before whole tile 5, workgroup 2)
    r.run(7)
    r.run(2000)
    r.to(3 * T + 64)
    r.run(5000)                       # tile 3 in pieces (before whole tile 6, workgroup 0) ...
    r.to(4 * T)                       # ... and its last k-mer ends a run: the next begins on J0 of tile 4, turn 1 of workgroup 1
    r.to(7 * T)                       # tiles 4 5 6 whole, one run from J0 of tile 4 to J0 of tile 7: the run workgroup 1 carries into its
    r.run(1000)                       # turn 2 ends exactly where that tile begins (J0 == v1)
    for _ in range(120):              # tile 7: a run boundary in more than SIDE_LANES lanes (the side buffer overflows: set directly)
        r.run(21)
    r.to(8 * T + 300)
    r.run(13)                         # tile 8 in pieces (behind whole tile 5)
    r.run(4000)
    r.to(9 * T + 8)
    r.run(100)                        # tile 9 in pieces (behind whole tile 6)
    r.to(10 * T - 5)
    r.to(12 * T + 50)                 # tiles 10 (behind tile 7, workgroup 1) and 11 whole
    r.run(200)                        # tile 12: the partial last tile, turn 4 of workgroup 0
    r.run(1)
    return r


SEAM_CLAIMS = dict(boundary_on_j0=4, carried_run_ends_on_j0=7,run_ends_on_tile_end=3, whole_between_pieces=(5, 6), side_overflow_then_whole=7, lane_of_eight_runs=True,
                   gallop_from=1, partial_last_turn=4, bypass=True)


def carried_runs():
    "one run longer than 4 * GRID tiles: every workgroup carries it from turn to turn and reads the run table once"
    r = Runs()
    r.run(3)
    r.run(4 * GRID * TILE + TILE // 2)
    r.ones(2)
    r.run(40)
    return r


def count_runs(n_tiles):
    "n_tiles tiles, the last one of ONE k-mer: (n_tiles - 1) * TILE + 1 k-mers in two runs (n_tiles = 1: the one k-mer)"
    r = Runs()
    if n_tiles > 1:
        r.run(TILE // 2 + 3)
        r.to((n_tiles - 1) * TILE)
    r.run(1)
    return r


def seam_cases(k):
    "name -> (records, k, SEAM_FILTERS, claims)"
    out = {}
    rng = np.random.default_rng(5000 + k)
    out["seams"] = (seam_runs().records(rng, k), k, SEAM_FILTERS, dict(SEAM_CLAIMS))
    out["carried"] = (carried_runs().records(rng, k), k, SEAM_FILTERS, dict(carried_run=True))
    for n in (1, 2, 3, 4, 5):         # GRID - 1, GRID, GRID + 1 for the grids 1 (as far as it goes), 3 and 4
        out[f"tiles{n}"] = (count_runs(n).records(rng, k), k, SEAM_FILTERS, dict(n_tiles=n, last_tile_of_one=True))
    return out


# ---- the repeats of tests/test_gpu_parity.py, placed ------------------------------------------------------------------------------------
def _unit_buckets(unit, k):
    "the level-1 buckets a period-8 repeat puts its k-mers into, per seam filter; None unless its eight k-mers have eight indices"
    seq = unit * ((k + 7) // 8 + 2)
    out = {}
    for nbytes in SEAM_FILTERS:
        idx = indices(seq[:k + 7], k, nbytes)
        if np.unique(idx).size != 8:
            return None
        out[nbytes] = set((idx >> np.uint64(LEVEL1_SHIFT[nbytes])).tolist())
    return out


def repeat_case():
    """k = 24.  b"A" * 300000 and b"ACGTTGCA" * 40000 fill a level-1 bucket many times over: every tile of theirs but the first few
    finds its reservation past cap1.  Behind each comes a filler, a period-8 repeat of 4 * TILE + 100 k-mers whose eight k-mers fall
    into buckets that nothing else fills (1/8 of a tile each, about 4100 in all: within cap1's slack of 4096 over the mean, which
    the repeats raise), so that the last tile of a repeat -- reservation over -- is followed three tiles on, in the same workgroup
    of three, by a whole single-run tile whose reservations all fit.  Random tiles between the two put the two overflowing tiles into
    turns of different parity."""
    k = 24
    rng = np.random.default_rng(2403)
    taken = {nbytes: set() for nbytes in SEAM_FILTERS}
    for rep in REPEATS:
        for nbytes in SEAM_FILTERS:
            taken[nbytes] |= set((indices(rep[:k + 7], k, nbytes) >> np.uint64(LEVEL1_SHIFT[nbytes])).tolist())
    fillers = []
    while len(fillers) < 2:
        unit = bases(rng, 8)
        b = _unit_buckets(unit, k)
        if b is None or any(b[nbytes] & taken[nbytes] or len(b[nbytes]) < 8 for nbytes in SEAM_FILTERS):
            continue
        for nbytes in SEAM_FILTERS:
            taken[nbytes] |= b[nbytes]
        fillers.append((unit * ((4 * TILE + 100 + k - 1) // 8 + 1))[:4 * TILE + 100 + k - 1])
    head = bases(rng, TILE + 2500 + k - 1)
    tail = bases(rng, TILE // 2 + k - 1)
    for gap_tiles in range(7):
        gap = bases(rng, gap_tiles * TILE + 777 + k - 1)
        records = [head, REPEATS[0], fillers[0], gap, REPEATS[1], fillers[1], tail]
        first = np.concatenate([[0], np.cumsum([len(s) - k + 1 for s in records])])
        last_tile = [int(first[i + 1] - 1) // TILE for i in (1, 4)]             # the last tile that holds k-mers of each repeat
        if (last_tile[0] // GRID) % 2 != (last_tile[1] // GRID) % 2:
            return records, k, SEAM_FILTERS, dict(overflow_then_ordinary=tuple(last_tile), bypass=True)
    raise AssertionError("no spacing puts the two overflowing tiles into turns of different parity")


# ---- the geometry cases -----------------------------------------------------------------------------------------------------------------
MIB = 1 << 20
# nbytes -> (what the fixed plan makes of it, (first index, last index + 1, at least this many searched k-mers) or None)
GEOMETRY = {
    32 * MIB: ("F = 512: one level, B1 = 512", None),
    32 * MIB + 8: ("F = 513: B2 = 2, B1 = 257, one bucket behind the filter's end", None),
    32 * MIB + 13: ("two levels, a partial last word behind packed words", "last_word"),
    32 * MIB + 11: ("two levels, three words in the last bucket: the scalar tails behind packed words", "last_word"),
    64 * MIB: ("F = 1024: B2 = 2, B1 = 512", None),
    64 * MIB + 8: ("F = 1025: B2 = 4, B1 = 257 (513 under the floor)", None),
    1025 * 65536 - 8: ("F = 1025, the last real bucket nearly full", "last_bucket"),
    3 * MIB + 12: ("one level, F = 49, three words in the last bucket", "last_word"),
    (1 << 29) + 8: ("F = 8193: more than 2^32 bits, FastMod form 2, B2 = 32", None),
}
GEOMETRY_K = 24
MIN_COUNT = {"last_word": 2, "last_bucket": 64}


def target_range(nbytes, what):
    "the filter indices [lo, hi) of `what`: the filter's last 4-byte word, or its last final bucket"
    bits = nbytes * 8
    if what == "last_word":
        return ((nbytes + 3) // 4 - 1) * 32, bits
    return ((bits - 1) >> FINAL_SHIFT) << FINAL_SHIFT, bits


_searched = {}
SEARCHED_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bloom_searched_kmers.json")


def searched_kmers():
    """nbytes -> list of k-mers (records of GEOMETRY_K bases) whose index lies in the case's target range: the recorded result of
    search_kmers() (tests/golden/bloom_searched_kmers.json; the host test holds the file against the search and every k-mer against
    the oracle's hash)"""
    if not _searched:
        with open(SEARCHED_FIXTURE, encoding="ascii") as fh:
            _searched.update({int(nbytes): [s.encode("ascii") for s in kmers] for nbytes, kmers in json.load(fh).items()})
    return _searched


def search_kmers():
    """What the fixture records: one walk over a fixed-seed random sequence, hashed by the oracle, until every case has its count (the
    rarest, eight bits of 2^28, takes tens of millions of k-mers)"""
    _searched = {}
    k = GEOMETRY_K
    want = {nbytes: (target_range(nbytes, what), MIN_COUNT[what]) for nbytes, (_, what) in GEOMETRY.items() if what}
    found = {nbytes: [] for nbytes in want}
    rng = np.random.default_rng(190)
    chunk = 1 << 24
    for _ in range(64):
        seq = bases(rng, chunk)
        pos, h0 = O.hash_all(seq, k)
        for nbytes, ((lo, hi), need) in want.items():
            if len(found[nbytes]) >= need:
                continue
            idx = h0 % np.uint64(nbytes * 8)
            for p in pos[(idx >= np.uint64(lo)) & (idx < np.uint64(hi))][:need - len(found[nbytes])]:
                found[nbytes].append(seq[int(p):int(p) + k])
        if all(len(found[nbytes]) >= need for nbytes, (_, need) in want.items()):
            _searched.update(found)
            return _searched
    raise AssertionError("the search did not fill every target range")


_base = {}


def geometry_base():
    "about 300 k random k-mers in a few records with N runs, a second small genome, and the first one's relative at 2 %"
    if not _base:
        rng = np.random.default_rng(411)
        seqs = []
        for n in (200000, 0, 30, 100001):
            a = np.frombuffer(bases(rng, n), dtype=np.uint8).copy()
            for at in rng.integers(0, max(n - 60, 1), size=n // 40000):
                a[at:at + int(rng.integers(1, 50))] = ord("N")
            seqs.append(a.tobytes())
        rel = []
        for s in seqs:
            a = np.frombuffer(s, dtype=np.uint8).copy()
            hit = (rng.random(a.size) < 0.02) & (a != ord("N"))
            a[hit] = ACGT[rng.integers(0, 4, size=int(hit.sum()))]
            rel.append(a.tobytes())
        _base.update(seqs=seqs, relative=rel, second=[bases(rng, 40000), bases(rng, 9000)])
    return _base


def geometry_case(nbytes):
    "(records, k, nbytes, claims) and the two other genomes of the case: (second, relative); the searched k-mers are in all three"
    what, target = GEOMETRY[nbytes]
    base = geometry_base()
    extra = list(searched_kmers()[nbytes]) if target else []
    claims = dict(shape=what)
    if target:
        claims[target] = MIN_COUNT[target]
    return (base["seqs"] + extra, GEOMETRY_K, nbytes, claims), (base["second"] + extra[:1], base["relative"] + extra)


# ---- the case without switches ----------------------------------------------------------------------------------------------------------
PRODUCT_FILTER = 32 * MIB + 8


def product_case(cus):
    """k_bin1's own grid of 2 * cus workgroups, 2 * grid + 3 tiles: every workgroup takes two tiles, three take a third.  One record of
    random bases; N runs break tiles b, b + grid and b + 2 * grid into pieces for b = 1 and b = 2 (the three turns of two workgroups),
    three of them in each."""
    k, grid = 24, 2 * cus
    n_tiles = 2 * grid + 3
    rng = np.random.default_rng(7000 + cus)
    a = np.frombuffer(bases(rng, n_tiles * TILE - 1234 + k - 1), dtype=np.uint8).copy()
    broken = [b + t * grid for b in (1, 2) for t in range(3)]
    shift = 0                                                     # every N run takes k - 1 + its length k-mers out: place from the left
    for t in sorted(broken):
        for j, off in enumerate((700, 2900, 5111)):
            at = t * TILE + off + shift + k                       # base position: compact index + the k-mers lost so far
            n = 1 + j
            a[at:at + n] = ord("N")
            shift += k - 1 + n
    return [a.tobytes()], k, PRODUCT_FILTER, dict(broken_tiles=tuple(broken), grid=grid, n_tiles=n_tiles)


# ---- a family of three genomes of any size ----------------------------------------------------------------------------------------------
def family(seed, n_bases, second=(40000, 9000)):
    """geometry_base()'s three genomes at another size: about n_bases random k-mers in a few records with N runs (one record empty, one
    of 30 bases), a second small genome, and the first one's relative at 2 %"""
    rng = np.random.default_rng(seed)
    seqs = []
    for n in (n_bases * 2 // 3, 0, 30, n_bases - n_bases * 2 // 3 + 1):
        a = np.frombuffer(bases(rng, n), dtype=np.uint8).copy()
        for at in rng.integers(0, max(n - 60, 1), size=min(n // 40000, 8)):
            a[at:at + int(rng.integers(1, 50))] = ord("N")
        seqs.append(a.tobytes())
    rel = []
    for s in seqs:
        a = np.frombuffer(s, dtype=np.uint8).copy()
        hit = (rng.random(a.size) < 0.02) & (a != ord("N"))
        a[hit] = ACGT[rng.integers(0, 4, size=int(hit.sum()))]
        rel.append(a.tobytes())
    return dict(seqs=seqs, relative=rel, second=[bases(rng, n) for n in second])


def hashes(records, k):
    "the oracle's first hash of every valid k-mer of a genome, record after record"
    return np.concatenate([O.hash_all(s, k)[1] for s in records] + [np.zeros(0, dtype=np.uint64)])


# ---- the second round of k_bin3's load loop ---------------------------------------------------------------------------------------------
# k_bin3 loads 4 * BIN3_THREADS 16-byte pieces per trip: 16384 unpacked residues (one partition level) or 8192 packed words of three
# residues each (two levels).  A final bucket takes a second trip with more than that.
BIN3_TRIP_RESIDUES, BIN3_TRIP_WORDS = 16384, 8192
SECOND_TRIP_K = 24
# name -> (nbytes, random k-mers of the first genome, REPEATS on top, seed, what the fixed plan makes of it)
SECOND_TRIP = {
    "one_bucket": (65536, 20000, False, 8810, "F = 1: one level, B1 = 1, cap1 about 26.6 k, the bucket of 20 k residues unclamped"),
    "two_buckets": (131072, 40000, False, 8811, "F = 2: one level, B1 = 2, 20 k residues each"),
    "two_buckets_over": (131072, 40000, True, 8816, "F = 2 with the repeats on top: a bucket clamped to cap1 > 16384, the rest set directly"),
    "packed": (32 * MIB + 8, 13_000_000, False, 8806, "F = 513: B2 = 2, B1 = 257, cap2 > 8192 words, every final bucket beyond 24 576 residues"),
}
_trip = {}


def second_trip_case(name):
    "(records, k, nbytes, claims) and (second, relative), as geometry_case(); the last case asked for is kept"
    if name not in _trip:
        _trip.clear()
        nbytes, n, over, seed, what = SECOND_TRIP[name]
        fam = family(seed, n, second=(n // 2, n - n // 2))    # (as many k-mers as the first: the read-and-OR finish takes the second trip too)
        extra = list(REPEATS) if over else []
        claims = dict(shape=what, overflow=over)
        _trip[name] = ((fam["seqs"] + extra, SECOND_TRIP_K, nbytes, claims), (fam["second"], fam["relative"] + extra))
    return _trip[name]


# ---- the large geometries: log2_b2 = 6 .. 9 ---------------------------------------------------------------------------------------------
GIB = 1 << 30


def partly_real(log2_b2):
    """a filter of 256 whole level-1 buckets and a 257th of which seven final buckets and 40013 bytes of an eighth are real (a partial
    last word too): the other 2^log2_b2 - 8 final buckets of that level-1 bucket lie behind the filter's end"""
    return ((256 << log2_b2) + 7) * 65536 + 40013


# nbytes -> what the fixed plan makes of it (tests/test_bloom_cases_host.py holds F, log2_b2, B2, B1, n_final against written-out numbers)
LARGE = {
    GIB + 8: "F = 16385: B2 = 64, B1 = 257 (513 under the floor), 63 buckets behind the filter's end",
    2 * GIB + 8: "F = 32769: B2 = 128, B1 = 257",
    4 * GIB + 8: "F = 65537: B2 = 256, B1 = 257",
    8 * GIB + 8: "F = 131073: B2 = 512, B1 = 257: every lane of k_bin2 clears and scans a counter",
    16 * GIB: "F = 262144: B2 = 512, B1 = 512, the largest geometry the plan accepts",
    partly_real(6): "F = 16392: B2 = 64, B1 = 257, the last level-1 bucket 8 real final buckets of 64, the last of them partial",
    partly_real(9): "F = 131080: B2 = 512, B1 = 257, the last level-1 bucket 8 real final buckets of 512, the last of them partial",
}
LARGE_K = 24
LARGE_PARTLY_REAL = (partly_real(6), partly_real(9))
_large = {}


def large_base():
    "family() at about 2 M k-mers and the hashes of its three genomes (first, second, relative), made once"
    if not _large:
        fam = family(977, 2_000_000)
        genomes = (fam["seqs"], fam["second"], fam["relative"])
        _large.update(genomes=genomes, h0=tuple(hashes(g, LARGE_K) for g in genomes))
    return _large


# ---- a filter as the set of its indices -------------------------------------------------------------------------------------------------
def sparse_reference(h0, nbytes):
    """The oracle's filter of nbytes bytes after each finish, as sorted arrays of distinct bit indices: insert of the first genome
    (the set of its indices), insert of the second (the union), the cascade level of the third (its indices that the running set
    holds: O.bf_build(..., prev=...) with one hash function).  h0: the three genomes' hashes (hashes())."""
    bits = np.uint64(nbytes * 8)
    first, second, third = (np.unique(h % bits) for h in h0)
    both = np.union1d(first, second)
    return first, both, np.intersect1d(third, both)


def sparse_bytes(idx):
    "(byte offsets, byte values) of the filter that holds exactly the bits of the sorted distinct indices idx: its non-zero bytes"
    byte = (idx >> np.uint64(3)).astype(np.int64)
    bit = np.left_shift(np.uint8(1), (idx & np.uint64(7)).astype(np.uint8))
    first = np.flatnonzero(np.concatenate(([True], byte[1:] != byte[:-1])))
    return byte[first], np.bitwise_or.reduceat(bit, first)

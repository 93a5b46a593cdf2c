"""Inputs for the sketch whose edge properties are CONSTRUCTED (tests/test_gpu_sketch_seams.py; checked on the CPU by
tests/test_sketch_cases_host.py): genomes whose runs of valid bases end, begin and tie on the seams of the tiles the sketch kernels cut
the compact k-mer index by, filters that leave a window uncovered on such a seam, and mask lists of every shape build_runs has to sort,
merge and clip.  Plain numpy, no GPU.

The tile sizes (ntsynt_amd/csrc): KEY_TILE 8192 (key array, dense pass, accept list), WIN_TILE 4096 windows (k_window_min), HIW_TILE 4096
per wave and SEL_TILE 16384 per workgroup (k_hash_select_hi / k_hash_select), 64 k-mers per lane, and the tiers' core = TR_EXT - 2 halo
with halo = ceil((w - 1) / 64) * 64.  A kernel that changes its tiling adds its tile size to default_tiles()."""
import numpy as np

from oracle import nts_oracle as O

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
LANE, WIN_TILE, HIW_TILE, KEY_TILE, SEL_TILE, TR_EXT = 64, 4096, 4096, 8192, 16384, 16384
TIER_MAX_W = 4097                      # the tiered selection applies up to this window (plan_sketch)
DS = (-1, 0, 1)
REC_SIZES = (("rec_w-1", -1), ("rec_w", 0), ("rec_w+1", 1))


def tier_core(w):
    return TR_EXT - 2 * (((w - 1 + 63) // 64) * 64)


def default_tiles(w):
    tiles = [LANE, WIN_TILE, KEY_TILE, SEL_TILE]
    if w <= TIER_MAX_W and tier_core(w) not in tiles:
        tiles.append(tier_core(w))
    return tiles


def rec_tile_ds(T):
    "a record of T + w - 2 + d k-mers has T - 1 + d windows: up to two beyond a full window tile where T is the window tile"
    return (-1, 0, 1, 2, 3) if T == WIN_TILE else DS


def expected_properties(w, tiles=None):
    "every (property, T, d) seam_genome places; T = 0: a property that belongs to no tile"
    tiles = default_tiles(w) if tiles is None else list(tiles)
    want = {(name, 0, 0) for name, _ in REC_SIZES} | {("empty_rec", 0, 0), ("short_rec", 0, 0)}
    for T in tiles:
        want |= {("run_end", T, d) for d in DS} | {("run_start", T, d) for d in DS} | {("tie", T, 0)}
        want |= {(name + "_end", T, d) for name, _ in REC_SIZES for d in DS}
        want |= {("rec_tile", T, d) for d in rec_tile_ds(T)}
    return want


# ---- the run arithmetic: valid k-mers in record order are the compact index ------------------------------------------------------------
class Layout:
    """Runs of valid k-mer starts of a list of records, as the oracle rolls them (O.hash_all: a k-mer is valid when its k bases are
    ACGT in either case) and as the library's run table lists them: run_first / run_n in compact indices, run_gpos the first k-mer's
    base counted over all records, rec_first / rec_nv per record."""

    def __init__(self, seqs, k):
        self.k = k
        self.rec_len = np.array([len(s) for s in seqs], dtype=np.int64)
        self.rec_off = np.concatenate([[0], np.cumsum(self.rec_len)]).astype(np.int64)
        gpos, n, rec = [], [], []
        for r, s in enumerate(seqs):
            if len(s) < k:
                continue
            a = np.frombuffer(s, dtype=np.uint8) & 0xDF
            bad = np.concatenate([[0], np.cumsum(~np.isin(a, ACGT))])
            ok = (bad[k:] - bad[:-k]) == 0                       # k-mer starting at p is valid
            edge = np.diff(np.concatenate([[0], ok.astype(np.int8), [0]]))
            starts, ends = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
            gpos.append(starts + self.rec_off[r])
            n.append(ends - starts)
            rec.append(np.full(starts.size, r))
        cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)
        self.run_gpos, self.run_n, self.run_rec = cat(gpos), cat(n), cat(rec)
        self.run_first = np.concatenate([[0], np.cumsum(self.run_n)])[:-1].astype(np.int64)
        self.run_last = self.run_first + self.run_n - 1
        self.n_valid = int(self.run_n.sum())
        self.rec_nv = np.bincount(self.run_rec, weights=self.run_n, minlength=len(seqs)).astype(np.int64)
        self.rec_first = np.concatenate([[0], np.cumsum(self.rec_nv)])[:-1].astype(np.int64)
        self.rec_runs = np.bincount(self.run_rec, minlength=len(seqs))

    def compact(self, rec, pos):
        "compact indices of the k-mers at (record, position)"
        g = self.rec_off[np.asarray(rec, dtype=np.int64)] + np.asarray(pos, dtype=np.int64)
        r = np.searchsorted(self.run_gpos, g, side="right") - 1
        out = self.run_first[r] + (g - self.run_gpos[r])
        assert ((g - self.run_gpos[r]) < self.run_n[r]).all()
        return out

    def gpos_of(self, idx):
        "base (counted over all records) at which the k-mers with these compact indices begin, and their run"
        idx = np.asarray(idx, dtype=np.int64)
        r = np.searchsorted(self.run_first, idx, side="right") - 1
        return self.run_gpos[r] + (idx - self.run_first[r]), r


def hashes(genome, k):
    "h0 of every valid k-mer in compact order, from the oracle"
    parts = [O.hash_all(genome.record(r), k)[1] for r in range(len(genome.names))]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint64)


def accepted(bf, h0):
    "per k-mer: does the filter (uint8 array, one hash function: bit h0 % bits) hold it"
    idx = h0 % np.uint64(bf.size * 8)
    return ((bf[(idx >> np.uint64(3)).astype(np.int64)] >> (idx & np.uint64(7)).astype(np.uint8)) & 1).astype(bool)


class Placed(list):
    "list of (property, T, d, compact index), with what it was computed for"
    k = w = 0
    tiles = ()
    layout = None


def find_placed(seqs, k, w, tiles=None):
    "what a genome holds on the seams, from its sequences alone"
    tiles = default_tiles(w) if tiles is None else list(tiles)
    lay = Layout(seqs, k)
    out = Placed()
    out.k, out.w, out.tiles, out.layout = k, w, tiles, lay
    single = lay.rec_runs == 1
    for r in np.flatnonzero(lay.rec_len == 0):
        out.append(("empty_rec", 0, 0, int(lay.rec_first[r])))
    for r in np.flatnonzero((lay.rec_len > 0) & (lay.rec_len < k)):
        out.append(("short_rec", 0, 0, int(lay.rec_first[r])))
    for name, e in REC_SIZES:
        for r in np.flatnonzero(single & (lay.rec_nv == w + e)):
            out.append((name, 0, 0, int(lay.rec_first[r])))
    blob = np.frombuffer(b"".join(seqs), dtype=np.uint8) & 0xDF
    change = np.flatnonzero(np.concatenate([[True], blob[1:] != blob[:-1], [True]]))
    stretch_end = change[np.searchsorted(change, np.arange(blob.size), side="right")] if blob.size else np.zeros(0, np.int64)
    for T in tiles:
        for d in DS:
            for prop, at in (("run_end", lay.run_last), ("run_start", lay.run_first)):
                hit = at[((at - d) % T == 0) & (at - d >= T)]
                out.extend((prop, T, d, int(x)) for x in hit)
            for name, e in REC_SIZES:
                last = lay.rec_first + lay.rec_nv - 1
                hit = np.flatnonzero(single & (lay.rec_nv == w + e) & ((last - d) % T == 0) & (last - d >= T))
                out.extend((name + "_end", T, d, int(last[r])) for r in hit)
        for d in rec_tile_ds(T):
            for r in np.flatnonzero(single & (lay.rec_nv == T + w - 2 + d)):
                out.append(("rec_tile", T, d, int(lay.rec_first[r])))
        # equal hashes on both sides of m T: the k-mers m T - 1 and m T of one run lie in one homopolymer stretch, and the bases behind
        # the stretch repeat with period two for k + 2 bases (the low-complexity neighbour)
        seams = np.arange(T, lay.n_valid, T, dtype=np.int64)
        if seams.size:
            g, r = lay.gpos_of(seams)
            inside = seams > lay.run_first[r]
            g, seams = g[inside] - 1, seams[inside]
            e = stretch_end[g]
            homo = e - g >= k + 1
            g, seams, e = g[homo], seams[homo], e[homo]
            for m, b in zip(seams, e):
                nb = blob[b:b + k + 2]
                if nb.size == k + 2 and nb[0] != nb[1] and (nb[2:] == nb[:-2]).all() and not np.isin(nb, ACGT, invert=True).any():
                    out.append(("tie", T, 0, int(m)))
    return out


# ---- the genome ------------------------------------------------------------------------------------------------------------------------
class _Builder:
    def __init__(self, k, rng):
        self.k, self.rng = k, rng
        self.records, self.cur, self.v, self.junk, self.joins = [], [], 0, 0, 0

    def random(self, n_kmers):
        a = ACGT[self.rng.integers(0, 4, size=n_kmers + self.k - 1)].copy()
        return a.tobytes()

    def end_record(self):
        if not self.cur:
            return
        self.records.append(b"".join(self.cur))
        self.cur = []
        self.junk += 1                                       # empty records and records shorter than k sit between the others
        if self.junk % 3 == 0:
            self.records.append(b"")
        if self.junk % 4 == 0:
            self.records.append(self.random(1)[:int(self.rng.integers(1, self.k))])
        if self.junk % 10 == 0:
            self.records.append(self.random(1)[:self.k - 1])

    def run(self, bases, new_record):
        "a run of len(bases) - k + 1 valid k-mers: behind a single N in the open record, or as the first run of a new one"
        assert len(bases) >= self.k
        if new_record:
            self.end_record()
        if self.cur:
            self.cur.append(b"N")
        self.cur.append(bases)
        self.v += len(bases) - self.k + 1

    def whole_record(self, n_kmers):
        self.end_record()
        self.run(self.random(n_kmers), True)
        self.end_record()

    def filler(self, n, pending):
        "n k-mers: the records that are needed somewhere and fit, then one random run"
        while True:
            fit = [x for x in pending if x <= n]
            if not fit:
                break
            x = max(fit)
            pending.remove(x)
            self.whole_record(x)
            n -= x
        if n:
            self.joins += 1
            self.run(self.random(n), self.joins % 2 == 0)


def seam_genome(k, w, tiles=None, rng=None):
    """(names, seqs, placed): see the module's docstring and expected_properties().  Seams are visited tile size by tile size, 4096
    first and the lanes' 64 last; a seam of 4096 that is one of 8192 or 16384 too counts for them (placed is computed from the sequences afterwards
    and lists it under every tile size it holds for)."""
    rng = np.random.default_rng(k * 100003 + w) if rng is None else rng
    tiles = default_tiles(w) if tiles is None else list(tiles)
    b = _Builder(k, rng)
    pending = [w + e for _, e in REC_SIZES] + [T + w - 2 + d for T in tiles for d in rec_tile_ds(T)]
    done = set()

    def seam_for(T, off, min_fill=0):
        "the first m T (m >= 1) with m T + off >= the cursor + min_fill; fills up to m T + off"
        m = max(1, -(-(b.v + min_fill - off) // T))
        b.filler(m * T + off - b.v, pending)
        return m * T

    def mark(M, props):
        for T2 in tiles:
            if M % T2 == 0:
                done.update((p, T2) for p in props)

    h = max(3, min(w // 2, 150))                             # equal hashes on either side of the seam
    n_ac = min(2 * w, 400)
    for T in sorted(tiles, key=lambda t: (t == LANE, t)):    # (every larger seam is one of 64 as well: the lanes come last and find theirs placed)
        # runs of one k-mer at m T - 1, m T and m T + 1: ends and starts at every d, through N cuts and record ends alternately
        if ("cluster", T) not in done:
            M = seam_for(T, -1, 1)
            for j in range(3):
                b.run(b.random(1), j % 2 == 1)
            b.run(b.random(int(rng.integers(5, 60))), True)
            mark(M, ["cluster"])
        # a long run that begins at m T - 1 (the records below begin long runs at m T, m T + 1 and m T + 2 and end them at every d)
        if ("start-1", T) not in done:
            M = seam_for(T, -1, 1)
            b.run(b.random(int(rng.integers(20, 80))), False)
            mark(M, ["start-1"])
        for name, e in REC_SIZES:
            for d in DS:
                if (name, d, T) in done:
                    continue
                n = w + e
                M = seam_for(T, d - n + 1)
                b.whole_record(n)
                assert b.v == M + d + 1
                for T2 in tiles:
                    if M % T2 == 0:
                        done.add((name, d, T2))
        if ("tie", T) not in done:
            pre = int(rng.integers(5, 40))
            M = seam_for(T, -(h + pre))
            body = bytearray(b.random(pre)[:pre])
            body[-1:] = b"G"
            body += b"A" * (2 * h + k - 1) + (b"CA" * (n_ac + k))[:n_ac + k] + b.random(int(rng.integers(10, 60)))
            b.joins += 1
            b.run(bytes(body), b.joins % 2 == 0)
            mark(M, ["tie"])
    b.filler(int(rng.integers(200, 400)), pending)
    for x in list(pending):
        b.whole_record(x)
    b.run(b.random(int(rng.integers(300, 600)) + w), True)
    b.end_record()
    seqs = b.records
    names = [f"s{i}" for i in range(len(seqs))]
    return names, seqs, find_placed(seqs, k, w, tiles)


# ---- the filter ------------------------------------------------------------------------------------------------------------------------
def seam_filter(og, k, nbytes, placed, keep=1):
    """The oracle's Bloom filter of the genome `og` (oracle container) with bits cleared so that, for every tile size T of `placed`,
    (a) at least w + 2 consecutive rejected k-mers of one record straddle a seam m T -- an uncovered window on the seam -- and
    (b) around another seam only the k-mers m T - 1 and m T are accepted, w + 1 rejected ones on either side where the record allows.
    keep > 1: a sparse filter (the accept list's regime) that holds one k-mer in `keep` to begin with.  Returns the filter (uint8)."""
    w, tiles, lay = placed.w, placed.tiles, placed.layout
    h0 = hashes(og, k)
    assert h0.size == lay.n_valid
    idx = (h0 % np.uint64(nbytes * 8)).astype(np.int64)
    if keep == 1:
        bits = np.unpackbits(O.bf_build(og, k, nbytes), bitorder="little").astype(bool)
    else:
        bits = np.zeros(nbytes * 8, dtype=bool)
        bits[idx[(h0 >> np.uint64(40)) % np.uint64(keep) == 0]] = True
    ties = np.array(sorted({i for p, _, _, i in placed if p == "tie"}), dtype=np.int64)
    used, pairs, gaps = [], [], []
    lo_all, hi_all = lay.rec_first, lay.rec_first + lay.rec_nv

    def candidates(T):
        out = []
        for lo, hi in zip(lo_all, hi_all):
            if hi - lo < w:
                continue
            m0, m1 = -(-(lo + 1) // T), (hi - 1) // T
            for m in (range(m0, m1 + 1) if m1 - m0 < 8 else sorted({m0, m0 + 1, (m0 + m1) // 2, m1 - 1, m1})):
                M = m * T
                if m >= 1 and lo < M < hi:
                    out.append((int(M), int(M - lo), int(hi - M)))
        return out

    def free(a, z):                                          # apart from the other stretches and from the seams with the equal hashes
        return all(z < ua or uz < a for ua, uz in used) and not ((ties >= a - min(w, 600)) & (ties < z + min(w, 600))).any()

    clear = np.zeros(bits.size, dtype=bool)                  # bits some rejected stretch relies on
    kept = []                                                # bits of the accepted pairs
    for T in tiles:                                          # (a) the uncovered window
        best = None
        for M, left, right in candidates(T):
            if left < 1 or right < 1 or left + right < w + 2:
                continue
            r_ = min(right, max(1, (w + 2) // 2))
            l_ = min(left, w + 2 - r_)
            r_ = w + 2 - l_
            if r_ > right or not free(M - l_, M + r_):
                continue
            score = (M % (2 * T) != 0, min(l_, r_))
            if best is None or score > best[0]:
                best = (score, M, l_, r_)
        if best is None:
            raise ValueError(f"no record straddles a seam of {T} with {w + 2} k-mers")
        _, M, l_, r_ = best
        clear[idx[M - l_:M + r_]] = True
        used.append((M - l_, M + r_))
        gaps.append((M - l_, M + r_))
    for T in tiles:                                          # (b) only m T - 1 and m T accepted
        best = None
        cand = candidates(T)
        for M, left, right, reach in ((M, left, right, reach) for reach in (w + 2, w // 4 + 3, 3) for M, left, right in cand):
            l_, r_ = min(left, reach), min(right, reach)
            if l_ < 3 or r_ < 3 or not free(M - l_, M + r_):
                continue
            around = np.concatenate([idx[M - l_:M - 1], idx[M + 1:M + r_]])
            if np.isin(idx[M - 1:M + 1], around).any() or clear[idx[M - 1:M + 1]].any() or np.isin(around, kept).any():
                continue
            score = (min(l_, r_), M % (2 * T) != 0)
            if best is None or score > best[0]:
                best = (score, M, l_, r_)
        if best is None:
            raise ValueError(f"no second seam of {T} for the accepted pair")
        _, M, l_, r_ = best
        clear[np.concatenate([idx[M - l_:M - 1], idx[M + 1:M + r_]])] = True
        kept += idx[M - 1:M + 1].tolist()
        used.append((M - l_, M + r_))
        pairs.append((M, l_, r_))
    bits[clear] = False
    for M, l_, r_ in pairs:
        bits[idx[M - 1:M + 1]] = True
    for M, l_, r_ in pairs:
        ok = bits[idx[M - l_:M + r_]]
        assert ok[l_ - 1] and ok[l_] and ok.sum() == 2, "an accepted pair shares a bit with a neighbour"
    for a, z in gaps:
        assert not bits[idx[a:z]].any()
    return np.packbits(bits, bitorder="little")


# ---- masks -----------------------------------------------------------------------------------------------------------------------------
def mask_lengths(k):
    return [80000, 40000, 4096 + k - 1, 100, 0]


def mask_family(k, rng, lengths=None):
    """(names, seqs, n_runs): records of `lengths` (default mask_lengths) with N at 0.3 % as tests.helpers.random_records places them,
    the first and last 300 bases of every record free of N, and two planted N runs of 40 per long record with 1500 clean bases on either
    side: n_runs lists the planted ones as (record, start, end)."""
    from tests.helpers import random_records
    lengths = mask_lengths(k) if lengths is None else lengths
    seqs, planted = [], []
    for r, s in enumerate(random_records(rng, lengths, n_frac=0.003)):
        a = np.frombuffer(s, dtype=np.uint8).copy()

        def clean(x, y):
            seg = a[x:y]
            bad = ~np.isin(seg & 0xDF, ACGT)
            seg[bad] = ACGT[rng.integers(0, 4, size=int(bad.sum()))]
        clean(0, 300)
        clean(max(0, a.size - 300), a.size)
        if a.size >= 30000:
            for at in (a.size // 3, 2 * a.size // 3):
                clean(at - 1500, at + 1540)
                a[at:at + 40] = ord("N")
                planted.append((r, at, at + 40))
        seqs.append(a.tobytes())
    return [f"m{i}" for i in range(len(seqs))], seqs, planted


def mask_sets(lengths, k, rng, n_runs=()):
    """Named lists of (rec, start, end) for records of `lengths`; n_runs: N runs (rec, start, end) with clean bases around them for the
    masks that abut an N run.  Yields (name, masks)."""
    long_recs = [r for r, n in enumerate(lengths) if n >= 4000]
    r0 = long_recs[0]
    base = []
    for r in long_recs:
        at = 400
        while at < lengths[r] - 4000:
            n = int(rng.integers(1, 3000))
            base.append((r, at, at + n))
            at += n + int(rng.integers(1, 2500))
    yield "sorted disjoint", list(base)
    yield "shuffled", [base[i] for i in rng.permutation(len(base))]
    dup = base + base
    yield "every interval twice", [dup[i] for i in rng.permutation(len(dup))]
    chains = []
    for c in range(6):
        a = 1000 + c * (lengths[r0] - 6000) // 6
        chains += [(r0, a + i * 50, a + i * 50 + int(rng.integers(51, 200))) for i in range(25)]
    yield "overlapping chains", [chains[i] for i in rng.permutation(len(chains))]
    yield "nested", [(r0, 1000, 5000), (r0, 2000, 3000),                 # inside one that ends later
                     (r0, 9000, 9500), (r0, 9200, 12000),                # begins inside one that ends earlier
                     (r0, 15000, 16000), (r0, 15000, 15100),             # the same start
                     (r0, 20000, 21000), (r0, 20900, 21000),             # the same end
                     (r0, 25000, 26000), (r0, 25000, 26000), (r0, 25001, 25999)]
    gaps = []
    for j, gap in enumerate((k - 1, k, k + 1)):
        a = 3000 + 7000 * j
        gaps += [(r0, a, a + 800), (r0, a + 800 + gap, a + 1700)]
    yield "pairs leaving k-1, k, k+1 bases", gaps
    assert len(long_recs) >= 3, "one record per gap"
    ends = []
    for r, gap in zip(long_recs, (k - 1, k, k + 1)):
        ends += [(r, lengths[r] - gap - 700, lengths[r] - gap), (r, gap, gap + 600)]   # the record's last and first `gap` bases stay
    yield "k-1, k, k+1 bases at record ends", ends
    if n_runs:
        sides = [(run, after) for run in n_runs for after in (True, False)]
        assert len(sides) >= 3, "one side of an N run per gap"
        near = []
        for ((r, s, e), after), gap in zip(sides, (k - 1, k, k + 1, k, k + 1, k - 1)):
            near.append((r, e + gap, e + gap + 500) if after else (r, s - gap - 500, s - gap))
        yield "k-1, k, k+1 bases beside an N run", near
        r, s, e = n_runs[0]
        yield "abutting and covering an N run", [(r, s - 200, s), (r, e, e + 150)] + [(r2, s2 - 10, e2 + 10) for r2, s2, e2 in n_runs[1:]]
    yield "empty and reversed", [(r0, 500, 500), (long_recs[-1], 900, 100), (r0, 0, 0), (r0, lengths[r0], lengths[r0])]
    beyond = [(r0, lengths[r0] - 1000, 10**12), (long_recs[-1], lengths[long_recs[-1]] + 10, lengths[long_recs[-1]] + 5000)]
    beyond += [(r, n, n + 100) for r, n in enumerate(lengths)] + [(r, 5, 10**9) for r, n in enumerate(lengths) if n < 5]
    yield "beyond the record", beyond
    yield "a whole record", [(long_recs[-1], 0, lengths[long_recs[-1]])]
    yield "all records", [(r, 0, n) for r, n in enumerate(lengths)]
    st = rng.integers(0, lengths[r0], size=2000)
    yield "2000 short masks", [(r0, int(s), int(s) + int(n)) for s, n in zip(st, rng.integers(1, 60, size=2000))]


def apply_masks(seqs, masks):
    "the records with every masked base turned into N (end clipped to the record; start >= end masks nothing)"
    out = [bytearray(s) for s in seqs]
    for r, st, en in masks:
        en = min(en, len(out[r]))
        if st < en:
            out[r][st:en] = b"N" * (en - st)
    return [bytes(b) for b in out]

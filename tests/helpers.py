"""Shared helpers for the parity tests: random sequences with the edge cases the domain has
(N runs, lower case, ragged / empty / short records) in both containers (oracle and HIP), and the oracle's statements of the
interval sweeps (counts, samples against a filter and against a set, sketches) that more than one module compares with."""
import numpy as np

from oracle import nts_oracle as O
from tests.divergence_ref import SENTINEL

U64_MAX = (1 << 64) - 1


def random_records(rng, lengths, n_frac=0.01, lower_frac=0.05, n_runs=True):
    seqs = []
    for ln in lengths:
        a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=ln)].copy()
        if ln and n_frac > 0:
            hit = rng.random(ln) < n_frac * 0.2
            a[hit] = ord("N")
            if n_runs and ln > 200:
                for _ in range(max(1, int(ln * n_frac / 200))):
                    st = int(rng.integers(0, ln - 50))
                    a[st:st + int(rng.integers(1, 400))] = ord("N")
        if ln and lower_frac > 0:
            for _ in range(max(1, ln // 5000)):
                st = int(rng.integers(0, max(1, ln - 10)))
                seg = a[st:st + int(rng.integers(1, 300))]
                seg[seg != ord("N")] |= 0x20
        seqs.append(a.tobytes())
    return seqs


def to_oracle(names, seqs):
    return O.Genome(names, seqs)


def to_device(ctx, names, seqs):
    from ntsynt_amd.device import Genome
    lens = np.array([len(s) for s in seqs], dtype=np.uint64)
    off = np.zeros(len(seqs), dtype=np.uint64)
    if len(seqs):
        off[1:] = np.cumsum(lens[:-1])
    blob = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    return Genome(ctx, names, blob, off, lens)


def oracle_flat(mins):
    "oracle per-record minimizers -> flat (h1, rec, pos) arrays like the device list"
    h = np.concatenate([m[0] for m in mins]) if mins else np.zeros(0, np.uint64)
    p = np.concatenate([m[1] for m in mins]) if mins else np.zeros(0, np.uint64)
    r = np.concatenate([np.full(len(m[0]), i, dtype=np.uint32) for i, m in enumerate(mins)]) \
        if mins else np.zeros(0, np.uint32)
    return h, r, p


END_CASE_KMERS = (1, 31, 33, 8191, 8192, 8193)     # one k-mer; a lane's share of 32 less and plus one; a tile of 8192 less, exactly, plus one


def genome_end_case(k):
    """(names, records, intervals) for the interval sweeps' partial lanes at the end of the genome: 30 000 bases in three records, the
    last one (20 000 bases, no N) ends the genome.  Intervals 0..5 hold exactly END_CASE_KMERS k-mers and end on the genome's last
    base, 6..11 hold the same numbers inside the record, and the last one straddles record 0's N run (3000..3040): its first piece,
    500 bases, ends in the middle of a lane for every k from 16 to 150."""
    rng = np.random.default_rng(1150)
    r0, r1, r2 = (bytearray(s) for s in random_records(rng, [6_000, 4_000, 20_000], n_frac=0.0, lower_frac=0.1))
    r0[3000:3040] = b"N" * 40
    seqs = [bytes(r0), bytes(r1), bytes(r2)]
    iv = [(2, 20_000 - (n + k - 1), 20_000) for n in END_CASE_KMERS]
    iv += [(2, 7 + 100 * j, 7 + 100 * j + n + k - 1) for j, n in enumerate(END_CASE_KMERS)]
    iv.append((0, 2500, 3500))
    assert (500 - k + 1) % 32 not in (0, 1)
    return [f"e{i}" for i in range(3)], seqs, iv


# ---- the interval sweeps by their definitions: what the GPU modules compare with, exactly ---------------------------------------------
def oracle_counts(seqs, k, bits, intervals):
    "per interval (valid k-mers wholly inside, those the filter holds)"
    per_rec, out = {}, []
    for rec, start, end in intervals:
        if rec not in per_rec:
            pos, h0 = O.hash_all(seqs[rec], k)
            per_rec[rec] = (pos.astype(np.int64), np.array([O.bf_contains(bits, h) for h in h0], dtype=bool))
        pos, held = per_rec[rec]
        inside = (pos >= start) & (pos + k <= min(end, len(seqs[rec])))
        out.append((int(inside.sum()), int(held[inside].sum())))
    return out


_per_k = {}


def oracle_kmers(seqs, k, bits):
    "per record (positions, hashes, held by the filter), once per k and filter"
    key = (k, bits.tobytes())
    if key not in _per_k:
        out = []
        for s in seqs:
            pos, h0 = O.hash_all(s, k)
            out.append((pos.astype(np.int64), h0, np.array([O.bf_contains(bits, h) for h in h0], dtype=bool)))
        _per_k.clear()
        _per_k[key] = out
    return _per_k[key]


def oracle_sample(seqs, k, bits, intervals, rate):
    "(records, per-interval counts) by the definitions: valid, wholly inside, held, h0 <= (2^64 - 1) // rate"
    from ntsynt_amd.device import SAMPLE_DTYPE
    per_rec = oracle_kmers(seqs, k, bits)
    thresh = np.uint64(U64_MAX // rate)
    parts, counts = [], []
    for i, (rec, start, end) in enumerate(intervals):
        pos, h0, held = per_rec[rec]
        a = min(start, len(seqs[rec]))
        take = (pos >= a) & (pos + k <= min(end, len(seqs[rec]))) & held & (h0 <= thresh)
        part = np.zeros(int(take.sum()), dtype=SAMPLE_DTYPE)
        part["h0"], part["iv"], part["off"] = h0[take], i, pos[take] - a
        parts.append(part)
        counts.append(part.size)
    return np.concatenate(parts), np.array(counts, dtype=np.uint64)


def oracle_set_sample(per_rec, seqs, k, members, intervals, rate):
    "(records, per-interval counts) by the definitions: valid, wholly inside, h0 <= (2^64 - 1) // rate, h0 in the set"
    from ntsynt_amd.device import SAMPLE_DTYPE
    thresh = np.uint64(U64_MAX // rate)
    parts, counts = [], []
    for i, (rec, start, end) in enumerate(intervals):
        pos, h0 = per_rec[rec]
        a = min(start, len(seqs[rec]))
        take = (pos >= a) & (pos + k <= min(end, len(seqs[rec]))) & (h0 <= thresh) & np.isin(h0, members)
        part = np.zeros(int(take.sum()), dtype=SAMPLE_DTYPE)
        part["h0"], part["iv"], part["off"] = h0[take], i, pos[take] - a
        parts.append(part)
        counts.append(part.size)
    return np.concatenate(parts), np.array(counts, dtype=np.uint64)


def oracle_sketches(seqs, k, s, intervals):
    "per interval (its s smallest distinct hashes, ascending; its valid k-mers)"
    per_rec = {}
    sk, nk = [], []
    for rec, start, end in intervals:
        if rec not in per_rec:
            per_rec[rec] = O.hash_all(seqs[rec], k)
        pos, h0 = per_rec[rec]
        pos = pos.astype(np.int64)
        inside = (pos >= start) & (pos + k <= min(end, len(seqs[rec])))
        h = np.unique(h0[inside])
        sk.append(h[h != SENTINEL][:s])
        nk.append(int(inside.sum()))
    return sk, nk

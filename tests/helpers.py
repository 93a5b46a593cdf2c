"""Shared helpers for the parity tests: random sequences with the edge cases the domain has
(N runs, lower case, ragged / empty / short records) in both containers (oracle and HIP)."""
import numpy as np

from oracle import nts_oracle as O


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

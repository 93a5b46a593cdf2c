"""CPU reference of the bottom-s MinHash sketch (nts_minhash): the oracle's canonical ntHash of every valid k-mer of every
record, np.unique, the sentinel 2^64 - 1 dropped, the first s kept."""
import numpy as np

from oracle import nts_oracle as O

SENTINEL = np.uint64(0xFFFFFFFFFFFFFFFF)


def ref_sketch(seqs, k, s):
    "seqs: the records (bytes) of one genome"
    parts = [O.hash_all(q, k)[1] for q in seqs]
    h = np.unique(np.concatenate(parts)) if parts else np.zeros(0, np.uint64)
    return h[h != SENTINEL][:s]

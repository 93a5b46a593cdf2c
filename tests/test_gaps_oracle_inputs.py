"""The inputs of tests/test_gpu_gaps.py's comparison with the oracle, checked where no GPU is: with the filter of the mutated copy
built by the oracle, the oracle's own counts over the test's intervals satisfy 0 < hits < k-mers at every k -- the divergence and the
filter size are chosen so that a match on the GPU is never vacuous."""
import numpy as np
import pytest

from oracle import nts_oracle as O
from tests import test_gpu_gaps as T


@pytest.mark.parametrize("k", T.KS)
def test_the_oracle_alone_sees_hits_and_misses(k):
    names, seqs, copy = T.oracle_inputs()
    bits = O.bf_build(O.Genome(names, copy), k, T.FILTER_BYTES)
    iv = T.intervals_for(k, seqs)
    ref = T.oracle_counts(seqs, k, bits, iv)
    total_k, total_h = sum(r[0] for r in ref), sum(r[1] for r in ref)
    occ = float(np.unpackbits(bits).sum()) / (bits.size * 8)
    print(f"k {k}: {total_h} of {total_k} k-mers held, occupancy {occ:.4f}")
    assert 0 < total_h < total_k
    assert occ < 0.5 and total_h / total_k > occ                # more than false positives alone: some k-mers survive the substitutions
    assert any(h == 0 and n > 0 for n, h in ref) or any(0 < h < n for n, h in ref)

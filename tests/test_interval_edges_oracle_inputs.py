"""The inputs of tests/test_gpu_interval_edges.py, checked where no GPU is: with the filter of the mutated copy built by the oracle,
the oracle's own figures over the test's intervals satisfy every condition that keeps a match on the GPU from being vacuous -- the
intervals hold the k-mers they are meant to hold, the filter holds some and misses some, the three rates and the hash set thin the
sample out but not to nothing, and the last lane of every full tile has k-mers whose loss would show."""
import numpy as np
import pytest

from oracle import nts_oracle as O
from tests import test_gpu_interval_edges as T
from tests.helpers import U64_MAX, genome_end_case, oracle_counts


def _figures(names, seqs, copy, iv, k, nbytes):
    bits = O.bf_build(O.Genome(names, copy), k, nbytes)
    per_rec = [(p.astype(np.int64), h) for p, h in (O.hash_all(s, k) for s in seqs)]
    held = [np.array([O.bf_contains(bits, h) for h in h0], dtype=bool) for _, h0 in per_rec]
    members = T.set_members(copy, k)
    inside = [(per_rec[rec][0] >= start) & (per_rec[rec][0] + k <= min(end, len(seqs[rec]))) for rec, start, end in iv]
    sizes = {rate: sum(int((m & held[row[0]] & (per_rec[row[0]][1] <= np.uint64(U64_MAX // rate))).sum()) for row, m in zip(iv, inside)) for rate in T.RATES}
    in_set = sum(int((m & np.isin(per_rec[row[0]][1], members)).sum()) for row, m in zip(iv, inside))
    return bits, per_rec, held, sizes, in_set


@pytest.mark.parametrize("k", T.KS)
def test_the_oracle_alone_satisfies_the_conditions(k):
    names, seqs, copy = T.edge_inputs()
    iv, want = T.edge_intervals(k)
    bits, per_rec, held, sizes, in_set = _figures(names, seqs, copy, iv, k, T.FILTER_BYTES)
    ref = oracle_counts(seqs, k, bits, iv)
    assert [r[0] for r in ref] == want
    total_k, total_h = sum(r[0] for r in ref), sum(r[1] for r in ref)
    occ = float(np.unpackbits(bits).sum()) / (bits.size * 8)
    print(f"k {k}: {total_h} of {total_k} k-mers held, occupancy {occ:.4f}; records at rates {sizes}, in the set {in_set}")
    assert 0 < total_h < total_k and sizes[1] == total_h
    assert occ < 0.5 and total_h / total_k > occ                # more than false positives alone: some k-mers survive the substitutions
    assert 0 < sizes[16] < sizes[3] < sizes[1]
    assert 0 < in_set < total_k
    for row in iv[:T.N_FULL]:
        n_held, n_unsampled = T.last_lane(k, per_rec, held, row)
        assert n_held > 0 and n_unsampled > 0, (row, n_held, n_unsampled)
    assert len({row[1] % 16 for row in iv[:T.N_FULL]}) == 16


@pytest.mark.parametrize("k", T.SMALL_KS)
def test_what_holds_at_k_1_and_2(k):
    "2 (10) canonical k-mers: the copy holds them all and their hashes are constants, so the conditions take the form they can"
    names, seqs, copy = T.edge_inputs()
    iv, want = T.edge_intervals(k)
    bits, per_rec, held, sizes, in_set = _figures(names, seqs, copy, iv, k, T.FILTER_BYTES)
    ref = oracle_counts(seqs, k, bits, iv)
    assert [r[0] for r in ref] == want and sum(want) > 0
    assert np.unique(np.concatenate([h for _, h in per_rec])).size == (2 if k == 1 else 10)
    assert all(h.all() for h in held) and 0 == sizes[16] <= sizes[3] <= sizes[1] == sum(want) and in_set == 0


@pytest.mark.parametrize("k", T.KS)
def test_the_end_of_the_genome_at_the_staging_limit(k):
    from ntsynt_amd import synth
    names, seqs, iv = genome_end_case(k)
    copy = [c.tobytes() for c in synth.derive_genome([np.frombuffer(s, dtype=np.uint8) for s in seqs], T.SUBSTITUTIONS, 1, seed=79, structural=False)]
    bits, _, _, sizes, in_set = _figures(names, seqs, copy, iv, k, 1 << 16)
    ref = oracle_counts(seqs, k, bits, iv)
    total_k, total_h = sum(r[0] for r in ref), sum(r[1] for r in ref)
    assert 0 < total_h < total_k and 0 < sizes[16] < sizes[3] < sizes[1] == total_h and 0 < in_set < total_k

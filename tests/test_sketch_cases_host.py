"""tests/sketch_cases.py delivers what tests/test_gpu_sketch_seams.py relies on -- checked without a GPU, so that the GPU tests cannot
quietly cover nothing: every (property, tile size, d) is on its seam, the oracle's list has minimizers on both sides of a seam of every
tile size and the seam filter leaves a window uncovered across one, and apply_masks is the N-substitution."""
import numpy as np
import pytest

from oracle import nts_oracle as O
from tests import sketch_cases as SC
from tests.helpers import oracle_flat, to_oracle

KS = [20, 24, 129]
WS = [10, 63, 64, 100, 250, 1000, 4097, 12000]
_cache = {}


def genome(k, w):
    if (k, w) not in _cache:
        _cache.clear()
        _cache[(k, w)] = SC.seam_genome(k, w)
    return _cache[(k, w)]


@pytest.mark.parametrize("w", WS)
@pytest.mark.parametrize("k", KS)
def test_every_property_is_on_every_seam(k, w):
    names, seqs, placed = genome(k, w)
    assert sum(len(s) for s in seqs) < 1_000_000
    have = {(p, T, d) for p, T, d, _ in placed}
    missing = SC.expected_properties(w) - have
    assert not missing, sorted(missing)
    assert set(placed.tiles) >= {64, 4096, 8192, 16384} and (w > SC.TIER_MAX_W or SC.tier_core(w) in placed.tiles)
    # placed is the sequences' own: the oracle rolls the same k-mers in the same order, and a listed index is what it says
    lay = placed.layout
    og = to_oracle(names, seqs)
    per_rec = [O.hash_all(s, k)[0] for s in seqs]
    assert [p.size for p in per_rec] == lay.rec_nv.tolist()
    for r in np.flatnonzero(lay.rec_nv)[:50]:
        assert np.array_equal(lay.compact(np.full(per_rec[r].size, r), per_rec[r]), lay.rec_first[r] + np.arange(per_rec[r].size))
    h0 = SC.hashes(og, k)
    for p, T, d, i in placed:
        if p == "tie":
            assert i % T == 0 and h0[i - 1] == h0[i]
        if p in ("run_end", "run_start"):
            assert (i - d) % T == 0 and (i in lay.run_last if p == "run_end" else i in lay.run_first)
    ties = [i for p, T, d, i in placed if p == "tie"]
    for i in ties[:5]:                                        # the neighbour, behind the k-mers that hold bases of both: two hashes in turn
        j = i
        while h0[j] == h0[i]:
            j += 1
        j += k
        assert h0[j] == h0[j + 2] == h0[j + 4] and h0[j] != h0[j + 1] and h0[j + 1] == h0[j + 3]


@pytest.mark.parametrize("w", WS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("keep", [1, 16])
def test_the_seam_filter_uncovers_a_window_on_a_seam_and_the_list_has_both_sides(k, w, keep):
    if keep == 16 and (k, w) not in ((24, 100), (24, 1000)):
        return                                                                    # (the sparse filter serves the accept list's two cells)
    names, seqs, placed = genome(k, w)
    lay = placed.layout
    og = to_oracle(names, seqs)
    nbytes = O.bf_ctor_bytes(O.bf_approx_bytes(og.total_bp, 0.025))
    bf = SC.seam_filter(og, k, nbytes, placed, keep=keep)
    h0 = SC.hashes(og, k)
    acc = SC.accepted(bf, h0)
    pick = np.random.default_rng(1).integers(0, h0.size, size=300)
    assert [O.bf_contains(bf, h0[i]) for i in pick] == acc[pick].tolist()
    assert (0.5 if keep == 1 else 0.02) < acc.mean() < (1.0 if keep == 1 else 0.2)
    h1, rec, pos = oracle_flat(O.minimize(og, k, w, bf))
    mins = lay.compact(rec, pos)
    assert (np.diff(mins) > 0).all() and acc[mins].all()
    is_min = np.zeros(lay.n_valid + 1, dtype=np.int64)
    is_min[mins + 1] = 1
    cum = np.cumsum(is_min)                                                       # cum[i] = minimizers below index i
    rec_of = np.repeat(np.arange(lay.rec_nv.size), lay.rec_nv)
    rej = np.concatenate([[0], np.cumsum(~acc)])
    new_rec = np.concatenate([[True], rec_of[1:] != rec_of[:-1]])
    run_a = np.flatnonzero(~acc & (new_rec | np.concatenate([[True], acc[:-1]])))     # stretches of rejected k-mers of one record: [run_a, run_z)
    run_z = np.flatnonzero(~acc & np.concatenate([new_rec[1:] | acc[1:], [True]])) + 1
    assert run_a.size == run_z.size
    for T in placed.tiles:
        M = np.arange(T, lay.n_valid - w, T)
        M = M[M >= w]
        both = (cum[M] - cum[M - w + 1] > 0) & (cum[M + w] - cum[M] > 0)
        assert both.any(), f"no seam of {T} with a minimizer closer than w on each side"
        # >= w + 2 rejected k-mers in a row, inside one record, m T among them but not the first
        seam_in = (-(-(run_a + 1) // T)) * T                                      # the first m T behind the stretch's first k-mer
        assert ((run_z - run_a >= w + 2) & (seam_in < run_z)).any(), f"no uncovered window across a seam of {T}"
        # only m T - 1 and m T accepted, both minimizers where w rejected k-mers of the record lie on either side
        pair = [m for m in M if acc[m - 1] and acc[m] and not acc[m - 2] and not acc[m + 1] and not acc[m - 3] and not acc[m + 2]]
        assert pair, f"no accepted pair on a seam of {T}"
        full = [m for m in pair if m + w + 1 <= lay.n_valid and rej[m - 1] - rej[m - 1 - w] == w and rej[m + 1 + w] - rej[m + 1] == w
                and rec_of[m - 1 - w] == rec_of[m + w]]
        for m in full:
            assert cum[m + 1] - cum[m - 1] == 2, f"the accepted pair on seam {m} of {T} is not in the list"


def test_apply_masks_is_the_n_substitution():
    k = 24
    rng = np.random.default_rng(5)
    names, seqs, n_runs = SC.mask_family(k, rng)
    lengths = [len(s) for s in seqs]
    assert lengths == SC.mask_lengths(k) and len(n_runs) == 4
    for r, s, e in n_runs:
        assert seqs[r][s:e] == b"N" * (e - s) and b"N" not in seqs[r][s - 1500:s].upper() + seqs[r][e:e + 1500].upper()
    sets = dict(SC.mask_sets(lengths, k, rng, n_runs))
    assert len(sets) == 14
    for name, masks in sets.items():
        got = SC.apply_masks(seqs, masks)
        for r, s in enumerate(seqs):
            m = np.zeros(len(s), dtype=bool)
            for _, a, b in (x for x in masks if x[0] == r):
                m[a:b] = True
            assert got[r] == np.where(m, ord("N"), np.frombuffer(s, dtype=np.uint8)).astype(np.uint8).tobytes(), name
    # the sets are what their names say
    assert sorted(sets["shuffled"]) == sets["sorted disjoint"] and sets["shuffled"] != sets["sorted disjoint"]
    assert sorted(sets["every interval twice"]) == sorted(sets["sorted disjoint"] * 2)
    assert all(a >= b or a >= lengths[r] for r, a, b in sets["empty and reversed"])
    assert SC.apply_masks(seqs, sets["empty and reversed"]) == seqs
    assert all(set(s) <= {ord("N")} for s in SC.apply_masks(seqs, sets["all records"]))
    lay = lambda sq: SC.Layout(sq, k)
    # a gap of k - 1 bases between two masks holds no k-mer, k one, k + 1 two
    gaps = sets["pairs leaving k-1, k, k+1 bases"]
    for pair, left in zip((gaps[0:2], gaps[2:4], gaps[4:6]), (0, 1, 2)):
        (r, s0, e0), (_, s1, e1) = pair
        masked = lay(SC.apply_masks(seqs, pair))
        inside = masked.run_gpos[(masked.run_gpos >= masked.rec_off[r] + e0) & (masked.run_gpos < masked.rec_off[r] + s1)]
        assert inside.size == (1 if left else 0)
        if left:
            assert masked.run_n[np.flatnonzero(masked.run_gpos == inside[0])[0]] == left

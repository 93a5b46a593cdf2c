"""Gap links on the GPU: nts_bf_sample_intervals (csrc/nts_bf_sample.inc) against the oracle -- O.hash_all of the record, the
threshold, O.bf_contains per k-mer -- record for record; the launch cut forced on the experiments build; nts_iv_links
(csrc/nts_iv_links.inc) against a brute force over dictionaries; `ntSynt --gap-links` and `bin/ntsynt_gaps --links-out` end to end
against a recomputation from gaps.cut, the oracle and the run's own .common.bf that calls nothing of gaps.links.  Every test runs
under a time limit of its own (a hung call ends the process, with a traceback)."""
import faulthandler
import os
import socket
import subprocess
import sys
from collections import Counter, defaultdict

import numpy as np
import pytest

from ntsynt_amd import assess, gaps, synth
from oracle import nts_oracle as O
from tests.helpers import END_CASE_KMERS, genome_end_case, oracle_sample, random_records, to_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STANDIN = os.path.join(ROOT, "tests", "rccl_standin", "librccl_standin.so")
STEP_SECONDS = 600
KS = [16, 24, 64, 150]
RATES = [1, 16, 1 << 20]
FILTER_BYTES = 1 << 17            # 1 M bits for 0.1 M k-mers: occupancy below 10 %
SUBSTITUTIONS = 0.02              # synth.derive_genome's pairwise figure: 1 % of the bases of the copy differ
U64_MAX = (1 << 64) - 1
N_RUN = (20_000, 20_050)          # record 0's only N run


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def ctx():
    from ntsynt_amd.device import Context
    c = Context(0)
    yield c
    c.close()


# ---- 1. sampling ----------------------------------------------------------------------------------------------------------------------
def sample_inputs():
    """(names, records, a mutated copy's records).  Record 0: 40 kbp without N but for one run, so that intervals of a chosen number of
    k-mers exist (a tile is 8192 k-mers of ONE stretch of valid bases), with a lower-case stretch; record 1: 30 kbp with an N every
    few hundred bases (many short pieces); record 2: 12 kbp."""
    rng = np.random.default_rng(410)
    r0, r2 = (bytearray(s) for s in random_records(rng, [40_000, 12_000], n_frac=0.0, lower_frac=0.1))
    r0[N_RUN[0]:N_RUN[1]] = b"N" * (N_RUN[1] - N_RUN[0])
    r2[6_000:6_001] = b"N"
    seqs = [bytes(r0), random_records(rng, [30_000], n_frac=0.02, lower_frac=0.1)[0], bytes(r2)]
    copy = synth.derive_genome([np.frombuffer(s, dtype=np.uint8) for s in seqs], SUBSTITUTIONS, 1, seed=78, structural=False)
    return [f"r{i}" for i in range(len(seqs))], seqs, [c.tobytes() for c in copy]


def sample_intervals(k):
    iv = [(0, 3 + 1000 * j, 3 + 1000 * j + n + k - 1) for j, n in enumerate((8191, 8192, 8193))]         # the tile's edge (19 345 < 20 000 at k = 150)
    iv += [(0, 21_001 + 500 * j, 21_001 + 500 * j + n + k - 1) for j, n in enumerate((31, 32, 33))]       # a lane's share
    iv += [(0, 100, 100 + k - 1),                                               # fewer than k bases
           (0, 19_700, 20_400),                                                 # across the N run: two pieces
           (0, 5_000, 9_000), (0, 7_000, 12_000), (0, 5_000, 9_000),            # overlapping; repeated
           (2, 11_000, 10**12),                                                 # clipped by the record's end
           (1, 0, 30_000),                                                      # many pieces
           (0, 20_050, 40_000),                                                 # three tiles, the last one short
           (1, 900, 900), (2, 13_000, 14_000)]                                  # empty; starts beyond the record
    return iv


def _filter_of(ctx, names, seqs, k, nbytes=FILTER_BYTES):
    from ntsynt_amd.device import BloomFilter
    g = to_device(ctx, names, seqs)
    bf = BloomFilter(ctx, nbytes, k)
    try:
        bf.insert(g)
    finally:
        g.free()
    return bf


@pytest.mark.parametrize("k", KS)
def test_samples_equal_the_oracle(ctx, k):
    from ntsynt_amd.device import SAMPLE_DTYPE
    names, seqs, copy = sample_inputs()
    bf = _filter_of(ctx, names, copy, k)
    g = to_device(ctx, names, seqs)
    try:
        bits = bf.to_numpy()
        iv = sample_intervals(k)
        kmers, hits = g.bf_count_intervals(bf, iv, k)
        assert [int(x) for x in kmers[:6]] == [8191, 8192, 8193, 31, 32, 33] and int(kmers[6]) == 0, k    # the intervals are what they are for
        for rate in RATES:
            got, counts = g.bf_sample_intervals(bf, iv, k, rate)
            exp, exp_counts = oracle_sample(seqs, k, bits, iv, rate)
            print(f"k {k} rate {rate}: {got.size} records, oracle {exp.size}; per interval {[int(c) for c in counts]}")
            assert got.dtype == SAMPLE_DTYPE and counts.dtype == np.uint64 and counts.shape == (len(iv),)
            assert np.array_equal(counts, exp_counts), (k, rate)
            assert got.size == exp.size and np.array_equal(got, exp), (k, rate)              # order, h0, iv and off
            if rate == 1:
                assert np.array_equal(counts, hits) and 0 < got.size < int(kmers.sum()), k       # never a vacuous match
                same = got[got["iv"] == 10].copy()
                same["iv"] = 8
                assert np.array_equal(got[got["iv"] == 8], same)                               # the repeated interval: the same records
            elif rate == 16:
                assert 0 < got.size < int(hits.sum()), k
            else:
                assert got.size <= 4, (k, got.size)                                            # 10^5 held k-mers, one in 2^20 sampled
        empty = g.bf_sample_intervals(bf, np.zeros((0, 3), np.uint64), k, 16)
        assert empty[0].size == 0 and empty[1].size == 0
    finally:
        g.free()
        bf.free()


@pytest.mark.parametrize("k", [150, 24])
def test_partial_lanes_up_to_the_last_base_of_the_genome(ctx, k):
    "k = 150: every lane reads its own bases and a partial one rolls on past the tile; k = 24: the same intervals through the staging area"
    names, seqs, iv = genome_end_case(k)
    copy = [c.tobytes() for c in synth.derive_genome([np.frombuffer(s, dtype=np.uint8) for s in seqs], SUBSTITUTIONS, 1, seed=79, structural=False)]
    bf = _filter_of(ctx, names, copy, k, nbytes=1 << 16)
    g = to_device(ctx, names, seqs)
    try:
        bits = bf.to_numpy()
        kmers, _ = g.bf_count_intervals(bf, iv, k)
        assert [int(x) for x in kmers[:12]] == list(END_CASE_KMERS) * 2, k
        for rate in (1, 16):
            got, counts = g.bf_sample_intervals(bf, iv, k, rate)
            exp, exp_counts = oracle_sample(seqs, k, bits, iv, rate)
            print(f"k {k} rate {rate}: {got.size} records, oracle {exp.size}; per interval {[int(c) for c in counts]}")
            assert np.array_equal(counts, exp_counts), (k, rate)
            assert got.size == exp.size and np.array_equal(got, exp), (k, rate)              # order, h0, iv and off
            assert 0 < got.size < int(kmers.sum()), (k, rate)                                # never a vacuous match
    finally:
        g.free()
        bf.free()


def test_full_and_empty_filters_and_a_bad_record_index(ctx):
    from ntsynt_amd.device import BloomFilter, NtsError
    names, seqs, _ = sample_inputs()
    g = to_device(ctx, names, seqs)
    ones = BloomFilter(ctx, FILTER_BYTES, 24, ones=True)
    zero = BloomFilter(ctx, FILTER_BYTES, 24)
    try:
        for k in KS:
            iv = sample_intervals(k)
            kmers, _ = g.bf_count_intervals(ones, iv, k)
            got, counts = g.bf_sample_intervals(ones, iv, k, 1)
            assert kmers.sum() > 0 and np.array_equal(counts, kmers) and got.size == int(kmers.sum()), k   # every valid k-mer
            parts = []
            for i, (rec, start, end) in enumerate(iv):
                pos, h0 = O.hash_all(seqs[rec], k)
                a = min(start, len(seqs[rec]))
                inside = (pos.astype(np.int64) >= a) & (pos.astype(np.int64) + k <= min(end, len(seqs[rec])))
                parts.append((h0[inside], np.full(int(inside.sum()), i), pos[inside].astype(np.int64) - a))
            assert np.array_equal(got["h0"], np.concatenate([p[0] for p in parts])), k
            assert np.array_equal(got["iv"], np.concatenate([p[1] for p in parts])) and np.array_equal(got["off"], np.concatenate([p[2] for p in parts])), k
            got0, counts0 = g.bf_sample_intervals(zero, iv, k, 1)
            assert got0.size == 0 and not counts0.any(), k
        with pytest.raises(NtsError, match="record index out of range"):
            g.bf_sample_intervals(ones, [(0, 0, 10), (len(seqs), 0, 10)], 24, 16)
        with pytest.raises(NtsError, match="bad arguments"):
            g.bf_sample_intervals(ones, [(0, 0, 100)], 24, 0)
    finally:
        g.free()
        ones.free()
        zero.free()


# ---- 2. slicing -----------------------------------------------------------------------------------------------------------------------
def test_more_tiles_than_one_launch_takes_give_the_same_records(ctx_x, monkeypatch):
    names, seqs, copy = sample_inputs()
    k = 24
    bf = _filter_of(ctx_x, names, copy, k)
    g = to_device(ctx_x, names, seqs)
    try:
        iv = sample_intervals(k) + [(0, a, a + 700) for a in range(0, 38_000, 500)]       # many short intervals as well
        ctx_x.profile(2)
        try:
            before = [ctx_x.timing(t)[1] for t in ("bf_sample_count", "bf_sample_write")]
            plain = g.bf_sample_intervals(bf, iv, k, 4)
            one = [ctx_x.timing(t)[1] - b for t, b in zip(("bf_sample_count", "bf_sample_write"), before)]
            monkeypatch.setenv("NTS_BF_SAMPLE_SLICE", "7")
            cut = g.bf_sample_intervals(bf, iv, k, 4)
            many = [ctx_x.timing(t)[1] - b - o for t, b, o in zip(("bf_sample_count", "bf_sample_write"), before, one)]
        finally:
            ctx_x.profile(False)
        print(f"launches (count, write): {one} uncut, {many} with 7 tiles per launch")
        assert one == [1, 1] and many[0] == many[1] and many[0] > 10
        assert np.array_equal(plain[0], cut[0]) and np.array_equal(plain[1], cut[1])
        exp, exp_counts = oracle_sample(seqs, k, bf.to_numpy(), iv, 4)
        assert np.array_equal(cut[0], exp) and np.array_equal(cut[1], exp_counts) and exp.size > 0
    finally:
        g.free()
        bf.free()


def test_the_launch_knob_is_not_in_the_product_build(ctx, monkeypatch):
    names, seqs, copy = sample_inputs()
    bf = _filter_of(ctx, names, copy, 24)
    g = to_device(ctx, names, seqs)
    try:
        monkeypatch.setenv("NTS_BF_SAMPLE_SLICE", "7")
        ctx.profile(2)
        try:
            before = [ctx.timing(t)[1] for t in ("bf_sample_count", "bf_sample_write")]
            g.bf_sample_intervals(bf, sample_intervals(24), 24, 4)
            assert [ctx.timing(t)[1] - b for t, b in zip(("bf_sample_count", "bf_sample_write"), before)] == [1, 1]
        finally:
            ctx.profile(False)
    finally:
        g.free()
        bf.free()


# ---- 3. the join ----------------------------------------------------------------------------------------------------------------------
def brute_links(lists, min_anchors):
    """the definitions over dictionaries.  lists: per genome [(h0, iv, off)].  Returns [(list_a, iv_a, list_b, iv_b, anchors, fwd, rev,
    min_off_a, max_off_a, min_off_b, max_off_b)] sorted.  Anchors of a link are ordered by their offset in a, equal offsets (which one
    genome's sweep cannot produce within a link) by hash."""
    seen = [Counter(h for h, _, _ in lst) for lst in lists]
    where = defaultdict(list)
    for l, lst in enumerate(lists):
        for h, iv, off in lst:
            where[h].append((l, iv, off))
    anchors = defaultdict(list)
    for h, members in where.items():
        if any(c[h] > 1 for c in seen):
            continue                                                            # twice in one list: dropped for every pair
        for x in range(len(members)):
            for y in range(x + 1, len(members)):
                (la, iva, offa), (lb, ivb, offb) = members[x], members[y]       # (list order: `where` was filled list by list)
                anchors[(la, iva, lb, ivb)].append((offa, h, offb))
    out = []
    for key in sorted(anchors):
        a = sorted(anchors[key])
        if len(a) < min_anchors:
            continue
        fwd = sum(1 for p, q in zip(a, a[1:]) if q[2] > p[2])
        rev = sum(1 for p, q in zip(a, a[1:]) if q[2] < p[2])
        out.append(key + (len(a), fwd, rev, min(p[0] for p in a), max(p[0] for p in a), min(p[2] for p in a), max(p[2] for p in a)))
    return out


def device_links(ctx, lists, min_anchors):
    from ntsynt_amd.device import LINK_DTYPE, SAMPLE_DTYPE
    arrs = []
    for lst in lists:
        a = np.zeros(len(lst), dtype=SAMPLE_DTYPE)
        if lst:
            a["h0"] = np.array([r[0] for r in lst], dtype=np.uint64)
            a["iv"], a["off"] = [r[1] for r in lst], [r[2] for r in lst]
        arrs.append(a)
    got = ctx.iv_links(arrs, min_anchors)
    assert got.dtype == LINK_DTYPE
    return [tuple(int(v) for v in row) for row in got]


def test_links_of_hand_made_lists(ctx):
    H = lambda i: (0x9E3779B97F4A7C15 * (i + 1)) & U64_MAX                    # noqa: E731 -- distinct hashes all over the 64 bits
    m = 4                                                                       # min_anchors
    a, b, c = [], [], []
    # gap 0 of a <-> gap 2 of b: exactly m anchors, rising
    for j in range(m):
        a.append((H(j), 0, 10 * j))
        b.append((H(j), 2, 7 + 5 * j))
    # gap 1 of a <-> gap 0 of b: m - 1 anchors
    for j in range(m - 1):
        a.append((H(100 + j), 1, 3 * j))
        b.append((H(100 + j), 0, 3 * j))
    # gap 2 of a <-> gap 1 of b: perfectly reversed, 9 anchors
    for j in range(9):
        a.append((H(200 + j), 2, 11 * j))
        b.append((H(200 + j), 1, 1000 - 11 * j))
    # gap 3 of a <-> gap 3 of b: fwd == rev (up, down, up, down)
    for j, off_b in enumerate((10, 30, 20, 40, 25)):
        a.append((H(300 + j), 3, j))
        b.append((H(300 + j), 3, off_b))
    # a hash twice in a (dropped everywhere: it would have been the 5th anchor of the first link, and an anchor with c)
    a += [(H(400), 0, 500), (H(400), 4, 0)]
    b.append((H(400), 2, 600))
    c.append((H(400), 0, 0))
    # hashes in three lists: three pairs each (gap 5 of a, gap 5 of b, gap 1 of c)
    for j in range(m):
        a.append((H(500 + j), 5, j))
        b.append((H(500 + j), 5, 2 * j))
        c.append((H(500 + j), 1, 100 - j))
    # a one-anchor link (kept only with min_anchors 1) and two anchors with one offset in a (ordered by hash)
    a.append((H(600), 6, 42))
    c.append((H(600), 2, 24))
    a += [(H(700), 7, 5), (H(701), 7, 5), (H(702), 7, 9)]
    c += [(H(700), 3, 50), (H(701), 3, 40), (H(702), 3, 60)]                     # (fwd, rev) = (1, 1) or (2, 0): by which of the two comes first
    rng = np.random.default_rng(3)
    lists = [[lst[i] for i in rng.permutation(len(lst))] for lst in (a, b, c)]  # the join does not rely on the records' order
    for min_anchors in (m, 1, 3):
        exp = brute_links(lists, min_anchors)
        got = device_links(ctx, lists, min_anchors)
        print(f"min_anchors {min_anchors}: {got}")
        assert got == exp, min_anchors
    at4 = {r[:4]: r for r in brute_links(lists, m)}
    assert at4[(0, 0, 1, 2)][4:7] == (m, m - 1, 0) and (0, 1, 1, 0) not in at4
    assert at4[(0, 2, 1, 1)][4:7] == (9, 0, 8) and at4[(0, 3, 1, 3)][4:7] == (5, 2, 2)
    assert {(0, 5, 1, 5), (0, 5, 2, 1), (1, 5, 2, 1)} <= set(at4) and at4[(0, 5, 2, 1)][5:7] == (0, m - 1)
    at1 = {r[:4]: r for r in brute_links(lists, 1)}
    assert at1[(0, 6, 2, 2)][4:] == (1, 0, 0, 42, 42, 24, 24) and (0, 1, 1, 0) in at1
    assert not any(r[:4] in ((0, 4, 1, 2), (0, 0, 2, 0), (0, 4, 2, 0), (1, 2, 2, 0)) for r in at1.values())      # the hash a has twice
    # an empty list among them, a single list, and no input at all
    assert device_links(ctx, [lists[0], [], lists[2]], 1) == brute_links([lists[0], [], lists[2]], 1) != []
    assert device_links(ctx, [[], lists[1], []], 1) == []
    assert device_links(ctx, [lists[0]], 1) == [] and device_links(ctx, [], 1) == [] and device_links(ctx, [[], []], 1) == []


def test_links_of_random_lists_cross_many_workgroups(ctx):
    """4 lists, 75 gaps each, 2 * 10^5 records.  Gap perm_l[g] of list l draws its hashes from group g's range of 22 000 values: 3 % of a
    list's records meet their hash a second time in the list, two lists share about 20 hashes per group, a few per cent of which
    fall to the uniqueness rule."""
    rng = np.random.default_rng(77)
    n_groups, per_gap, width = 75, 667, 22_000
    lists = []
    for l in range(4):
        perm = rng.permutation(n_groups)
        ids = (np.arange(n_groups)[:, None] * width + rng.integers(0, width, size=(n_groups, per_gap))).ravel()
        h = (ids.astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)        # a bijection of the ids onto all 64 bits
        iv = np.repeat(perm, per_gap)
        off = rng.integers(0, 50_000, size=ids.size)
        order = rng.permutation(ids.size)
        lists.append([(int(a), int(b), int(c)) for a, b, c in zip(h[order], iv[order], off[order])])
        dup = 1 - np.unique(ids).size / ids.size
        print(f"list {l}: {ids.size} records, {dup:.3f} of them a repeated hash")
        assert 0.005 < dup < 0.05
    assert sum(len(x) for x in lists) > 200_000
    every = brute_links(lists, 1)
    strong = [r for r in every if r[4] >= 15]                                   # (the threshold only drops links)
    for min_anchors, exp in ((15, strong), (1, every)):
        got = device_links(ctx, lists, min_anchors)
        print(f"min_anchors {min_anchors}: {len(got)} links, brute force {len(exp)}")
        assert got == exp
    assert 100 < len(strong) < len(every) <= 6 * n_groups


# ---- 4. end to end --------------------------------------------------------------------------------------------------------------------
INSERT_AT, INSERT_BP = 90_000, 6_000           # genome 1 only, contig 1: sequence no other genome has
INVERT_AT, INVERT_BP = 200_000, 6_000          # genome 1 only, contig 1 (coordinates before the insertion): shared, but on the other strand
PARAMS = ["-d", "1", "-k", "24", "-w", "300", "--w_rounds", "100", "10", "--indel", "500", "--merge", "1000", "-b", "8000", "-p", "g"]
RATE, MIN_ANCHORS = 16, 4                      # the switches' defaults


def gap_family(outdir):
    """tests/test_gpu_gaps.py's family: three genomes of 2 x 300 kbp at 1 %, no rearrangements but two in genome 1: an insertion of
    random sequence and an inverted segment, both shorter than the shortest block reported (-b 8000)"""
    anc = synth.make_ancestor(600_000, 2, seed=21)
    fam = [synth.derive_genome(anc, 0.01, j, seed=21, structural=False) for j in range(3)]
    c = fam[1][0]
    c[INVERT_AT:INVERT_AT + INVERT_BP] = synth.revcomp(c[INVERT_AT:INVERT_AT + INVERT_BP])
    private = synth.random_dna(INSERT_BP, np.random.default_rng(5))
    fam[1][0] = np.concatenate([c[:INSERT_AT], private, c[INSERT_AT:]])
    paths = []
    for j, contigs in enumerate(fam):
        paths.append(os.path.join(outdir, f"fam{j}.fa"))
        synth.write_fasta(paths[-1], contigs)
    return paths, fam


def _run(cmd, cwd, env=None, timeout=900):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=timeout, env=env or dict(os.environ, PYTHONPATH=ROOT))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def recompute_links(blocks_tsv, common_bf, fam, names, rate, min_anchors):
    "(text of the links file, link rows, gaps) from gaps.cut, the oracle's hashes, the filter file and the definitions: no GPU, none of gaps.links"
    from ntsynt_amd.pipeline import read_bf
    bits, k = read_bf(common_bf)
    records = {name: [(f"chr{i + 1}", int(c.size)) for i, c in enumerate(contigs)] for name, contigs in zip(names, fam)}
    cut_gaps, _ = gaps.cut(assess.read_blocks(blocks_tsv), records)
    thresh = np.uint64(U64_MAX // rate)
    order = sorted(names)
    per_genome, lists, sampled = {}, [], []
    for name in order:
        contigs = fam[names.index(name)]
        mine = [g for g in cut_gaps if g.genome == name]
        per_genome[name] = mine
        kmers = {}
        for i, c in enumerate(contigs):
            pos, h0 = O.hash_all(c.tobytes(), k)
            low = h0 <= thresh
            pos, h0 = pos[low].astype(np.int64), h0[low]
            held = np.array([O.bf_contains(bits, h) for h in h0], dtype=bool)
            kmers[f"chr{i + 1}"] = (pos[held], h0[held])
        lst, cnt = [], []
        for q, g in enumerate(mine):
            pos, h0 = kmers[g.contig]
            inside = (pos >= g.start) & (pos + k <= g.end)
            lst += [(int(h), q, int(p) - g.start) for p, h in zip(pos[inside], h0[inside])]
            cnt.append(int(inside.sum()))
        lists.append(lst)
        sampled.append(cnt)
    rows = []
    for la, iva, lb, ivb, anchors, fwd, rev, min_a, max_a, min_b, max_b in brute_links(lists, min_anchors):
        a, b = per_genome[order[la]][iva], per_genome[order[lb]][ivb]
        fa, fb = {a.left_block, a.right_block}, {b.left_block, b.right_block}
        rows.append([a.genome, a.contig, a.start, a.end, a.left_block, a.right_block, b.genome, b.contig, b.start, b.end, b.left_block, b.right_block,
                     anchors, "+" if fwd > rev else "-" if rev > fwd else ".", a.start + min_a, a.start + max_a + k, b.start + min_b, b.start + max_b + k,
                     sampled[la][iva], sampled[lb][ivb], "same" if fa == fb and fa != {"."} else "other"])
    header = ("genome_a contig_a start_a end_a left_a right_a genome_b contig_b start_b end_b left_b right_b anchors orientation from_a to_a "
              "from_b to_b sampled_a sampled_b placement").split()
    text = "".join("\t".join(str(v) for v in r) + "\n" for r in [header] + rows)
    return text + f"# k {k}, rate {rate}, min_anchors {min_anchors}, filter {bits.size * 8} bits\n", rows, cut_gaps


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    "the family and three runs of it: plain, --gaps, --gap-links --benchmark"
    tmp = tmp_path_factory.mktemp("gap_links")
    paths, fam = gap_family(str(tmp))
    ntsynt = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")]
    dirs = {}
    for name, extra in (("plain", []), ("gaps", ["--gaps"]), ("links", ["--gap-links", "--benchmark"])):
        dirs[name] = tmp / name
        dirs[name].mkdir()
        r = _run(ntsynt + paths + PARAMS + extra, dirs[name])
        assert r.returncode == 0, r.stderr[-3000:]
    return tmp, paths, fam, dirs


def test_the_switch_adds_files_and_changes_none(runs):
    _, _, _, dirs = runs
    plain, with_gaps, with_links = dirs["plain"], dirs["gaps"], dirs["links"]
    expected_same = sorted(os.listdir(plain))
    assert "g.synteny_blocks.tsv" in expected_same and "g.common.bf" in expected_same
    for name in expected_same:
        assert (plain / name).read_bytes() == (with_links / name).read_bytes() and (plain / name).stat().st_size > 0, name
    assert sorted(set(os.listdir(with_links)) - set(expected_same)) == ["g.gap_links.tsv", "g.gap_summary.tsv", "g.gaps.tsv", "g.stage_times.tsv"]
    for name in ("g.gaps.tsv", "g.gap_summary.tsv"):
        assert (with_gaps / name).read_bytes() == (with_links / name).read_bytes() and (with_gaps / name).stat().st_size > 0, name
    assert not (with_gaps / "g.gap_links.tsv").exists()
    stages = [ln.split("\t")[0] for ln in (with_links / "g.stage_times.tsv").read_text().splitlines()]
    assert stages.index("gaps") < stages.index("gap_links")


def test_the_links_file_equals_a_recomputation(runs):
    _, paths, fam, dirs = runs
    names = [os.path.basename(p) for p in paths]
    out = dirs["links"]
    got = (out / "g.gap_links.tsv").read_text()
    print(got)
    text, rows, cut_gaps = recompute_links(str(out / "g.synteny_blocks.tsv"), str(out / "g.common.bf"), fam, names, RATE, MIN_ANCHORS)
    assert got.splitlines()[0].split("\t") == list(gaps.LINK_COLUMNS)
    assert got == text
    assert rows

    def gap_over(genome, a, b):
        best = max((g for g in cut_gaps if g.genome == genome and g.contig == "chr1"), key=lambda g: min(g.end, b) - max(g.start, a))
        assert min(best.end, b) - max(best.start, a) >= (b - a) * 0.8, (genome, a, b, best)      # the segment lies in ONE gap, not in a block
        return (best.genome, best.contig, best.start)
    ins = gap_over(names[1], INSERT_AT, INSERT_AT + INSERT_BP)
    inv = gap_over(names[1], INVERT_AT + INSERT_BP, INVERT_AT + INSERT_BP + INVERT_BP)
    ends = lambda r: ((r[0], r[1], r[2]), (r[6], r[7], r[8]))                   # noqa: E731
    of_inv = [r for r in rows if inv in ends(r)]
    partners = {}
    for r in of_inv:
        other = ends(r)[1] if ends(r)[0] == inv else ends(r)[0]
        partners.setdefault(other[0], []).append((other, r))
    print(f"links of the inversion's gap {inv}:")
    for r in of_inv:
        print("   ", r)
    assert sorted(partners) == [names[0], names[2]] and all(len(v) == 1 for v in partners.values())      # one gap in each of the other two
    for other, r in (v[0] for v in partners.values()):
        assert r[13] == "-" and r[20] == "same" and r[12] >= MIN_ANCHORS, r
        print(f"anchors of the inversion's gap with {other}: {r[12]}")
    g0, g2 = partners[names[0]][0][0], partners[names[2]][0][0]
    between = [r for r in rows if ends(r) == (g0, g2)]
    assert len(between) == 1 and between[0][13] == "+" and between[0][20] == "same" and between[0][12] >= MIN_ANCHORS, between
    print(f"anchors between the other two genomes' gaps there: {between[0][12]}")
    assert not [r for r in rows if ins in ends(r)]                              # the private insertion: nothing to link to


def test_the_tool_reproduces_the_file_and_is_unchanged_without_the_option(runs):
    tmp, paths, _, dirs = runs
    out = dirs["links"]
    tool = [sys.executable, os.path.join(ROOT, "bin", "ntsynt_gaps"), "--tsv", str(out / "g.synteny_blocks.tsv"), "--fastas"] + paths + \
           ["--common", str(out / "g.common.bf")]
    r = _run(tool + ["--out", str(tmp / "again.tsv"), "--summary-out", str(tmp / "again_summary.tsv"), "--links-out", str(tmp / "again_links.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp / "again_links.tsv").read_bytes() == (out / "g.gap_links.tsv").read_bytes()
    assert (tmp / "again.tsv").read_bytes() == (out / "g.gaps.tsv").read_bytes()
    assert (tmp / "again_summary.tsv").read_bytes() == (out / "g.gap_summary.tsv").read_bytes()
    before = set(os.listdir(tmp))
    r = _run(tool, tmp)
    assert r.returncode == 0 and r.stdout == (out / "g.gaps.tsv").read_text() + (out / "g.gap_summary.tsv").read_text(), r.stderr[-3000:]
    assert set(os.listdir(tmp)) == before
    # other settings through the tool: every anchor counted, a link from one anchor on
    r = _run(tool + ["--out", os.devnull, "--summary-out", os.devnull, "--links-out", str(tmp / "dense.tsv"), "--links-rate", "1", "--links-min", "1"], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    dense = (tmp / "dense.tsv").read_text().splitlines()
    assert dense[-1].startswith("# k 24, rate 1, min_anchors 1, ") and len(dense) >= len((out / "g.gap_links.tsv").read_text().splitlines())


def test_gap_links_is_refused_under_two_ranks_and_without_a_filter(tmp_path):
    paths = synth.make_family(str(tmp_path), 2, 200_000, 1, 0.01, seed=14)
    out = tmp_path / "out"
    out.mkdir()
    env = dict(os.environ, PYTHONPATH=ROOT, NTS_RCCL_LIB=STANDIN, MASTER_ADDR="127.0.0.1", NTS_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bin", "ntSynt")] + paths + ["-d", "1", "-p", "p", "--gap-links"]
    r = _run(cmd, out, env=env, timeout=300)
    assert r.returncode != 0
    assert "--gap-links works from the genomes resident on one GPU" in r.stderr
    assert os.listdir(out) == []
    r = _run([sys.executable, os.path.join(ROOT, "bin", "ntSynt")] + paths + ["-d", "1", "-p", "p", "--gap-links", "--no-common"], out)
    assert r.returncode != 0 and "--gap-links reads the common Bloom filter" in r.stderr and os.listdir(out) == []

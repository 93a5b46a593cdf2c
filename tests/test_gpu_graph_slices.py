"""The graph build over key ranges (csrc/nts_graph.hip, graph_build_core): forced into many hash-range slices by a small scratch
budget (Context.set_graph_budget) it must give the graph of the build with one range per pass bit for bit -- vertices, occurrences,
edges in ntJoin's dict order -- through nts_graph_build and through the device engine's adds across rounds, in less scratch; with
the automatic budget the builds that fit have one range, plan nothing and keep their buffers on the context."""
import os

import numpy as np
import pytest

from ntsynt_amd import synth
from oracle import synteny_oracle as SO

pytestmark = pytest.mark.gpu

PREFIX = np.uint64(0xA5C3) << np.uint64(48)


@pytest.fixture(scope="module")
def ctx():
    from ntsynt_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _family_lists(ctx, tmp_path, n_asm, seed, bp=1_200_000, w=120):
    """minimizer lists of a synthetic family, with repeats inside each assembly and a fifth of the hashes moved under one 16-bit
    prefix (a bin far over any small budget: split again on the next 16 bits).  The moves are functions of the hash, so hashes
    common to the assemblies stay common."""
    from ntsynt_amd import fasta as fa
    from ntsynt_amd.device import Genome, sketch
    os.makedirs(tmp_path / f"f{seed}")
    paths = synth.make_family(str(tmp_path / f"f{seed}"), n_asm, bp, 3, 0.01, seed=seed, micro=6)
    rng = np.random.default_rng(seed)
    out = []
    for p in paths:
        r = fa.read_fasta(p)
        g = Genome(ctx, r.names, r.seq, r.rec_off, r.rec_len)
        mx = sketch(ctx, g, 24, w)
        h, rec, pos = mx.to_numpy()
        mx.free()
        g.free()
        h = h.copy()
        hot = (h % np.uint64(5)) == 0
        h[hot] = (h[hot] & np.uint64((1 << 48) - 1)) | PREFIX
        dup = rng.choice(h.size, size=h.size // 50, replace=False)          # within-assembly repeats
        h[dup] = h[rng.choice(h.size, size=dup.size)]
        out.append((h, rec.astype(np.uint32), pos))
    return out


def _oracle_edges(lists):
    "SO.build_graph over the lists ntJoin's filter leaves: (vertex hashes ascending, [(s, t, weight)] in its edge order)"
    valid, sets = [], []
    for h, _, _ in lists:
        _, inv, cnt = np.unique(h, return_inverse=True, return_counts=True)
        ok = cnt[inv] == 1
        valid.append(ok)
        sets.append(set(h[ok].tolist()))
    common = set.intersection(*sets)
    list_mxs = {}
    for a, (h, rec, _) in enumerate(lists):
        runs, cur, last = [], [], None
        for x, r, ok in zip(h.tolist(), rec.tolist(), valid[a].tolist()):
            if r != last and cur:
                runs.append(cur)
                cur = []
            last = r
            if ok and x in common:
                cur.append(x)
        if cur:
            runs.append(cur)
        list_mxs[a] = runs
    g = SO.build_graph(list_mxs, {a: 1 for a in range(len(lists))})
    return np.array(sorted(common), dtype=np.uint64), [(e[0], e[1], e[2]) for e in g.edges]


def _graphs_equal(a, b):
    for f in ("v_hash", "occ_rec", "occ_pos", "e_u", "e_v", "e_w", "e_first"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


def _total(lists):
    return sum(len(x[0]) for x in lists)


@pytest.mark.parametrize("n_asm,seed", [(2, 41), (3, 42), (8, 43)])
def test_sliced_build_equals_one_pass_and_oracle(ctx, tmp_path, n_asm, seed):
    from ntsynt_amd.graph import build_graph_device
    lists = _family_lists(ctx, tmp_path, n_asm, seed, bp=1_200_000 if n_asm < 8 else 400_000)
    n = _total(lists)
    ctx.set_graph_budget(0)
    one = build_graph_device(ctx, lists)
    assert ctx.graph_last_plan()["v_slices"] == 1 and ctx.graph_last_plan()["e_slices"] == 1
    ctx.set_graph_budget(n * 70 // 8)                                      # about an eighth of the elements per slice
    try:
        sliced = build_graph_device(ctx, lists)
        plan = ctx.graph_last_plan()
    finally:
        ctx.set_graph_budget(0)
    assert plan["v_slices"] >= 4 and plan["e_slices"] >= 2, plan
    assert one.v_hash.size > 500 and one.e_u.size > 500
    _graphs_equal(sliced, one)
    v_hash, edges = _oracle_edges(lists)
    assert np.array_equal(one.v_hash, v_hash)
    got = list(zip(one.v_hash[one.e_u].tolist(), one.v_hash[one.e_v].tolist(), one.e_w.tolist()))
    assert got == edges


def test_keep_mask_and_list_ids_sliced(ctx, tmp_path):
    "the caller's keep mask and list ids (the host engine's refinement rounds) through the sliced build"
    from ntsynt_amd.graph import build_graph_device
    lists = _family_lists(ctx, tmp_path, 3, 44)
    rng = np.random.default_rng(5)
    keeps = [rng.random(len(x[0])) < 0.97 for x in lists]
    lids = [(x[1].astype(np.int64) * 1000 + np.cumsum(rng.random(len(x[0])) < 0.01)).astype(np.uint32) for x in lists]
    one = build_graph_device(ctx, lists, keeps, lids)
    ctx.set_graph_budget(_total(lists) * 70 // 16)
    try:
        sliced = build_graph_device(ctx, lists, keeps, lids)
        assert ctx.graph_last_plan()["v_slices"] >= 8
    finally:
        ctx.set_graph_budget(0)
    _graphs_equal(sliced, one)


def _engine_state(g):
    return {f: g.read(f) for f in ("v_hash", "v_alive", "v_rec", "v_pos", "internal", "terminal", "e_u", "e_v", "e_w", "e_alive")}


def _states_equal(a, b, what):
    sa, sb = _engine_state(a.graph), _engine_state(b.graph)
    for f in sa:
        assert np.array_equal(sa[f], sb[f]), (what, f)


def test_device_engine_in_lockstep_with_slicing_forced(ctx, tmp_path):
    """Two device engines on one family through the initial round and two refinement rounds (block-interior spans, adds onto a
    non-empty graph, edges that exist already): one builds with a tiny budget, one with the automatic one; the state is the same
    after every step."""
    from ntsynt_amd import fasta as fa
    from ntsynt_amd.device import BloomFilter, Genome, bf_size_bytes, sketch
    from ntsynt_amd.synteny_device import DeviceSyntenyEngine
    n, k, w, rounds = 3, 24, 1000, [100, 10]
    paths = synth.make_family(str(tmp_path), n, 3_000_000, 3, 0.01, seed=21, micro=0, n_runs=True)
    recs = [fa.read_fasta(p) for p in paths]
    genomes = [Genome(ctx, r.names, r.seq, r.rec_off, r.rec_len) for r in recs]
    _, nbytes = bf_size_bytes(genomes[sorted(range(n), key=lambda i: paths[i])[0]].total_bp, 0.025)
    bf = BloomFilter(ctx, nbytes, k)
    tmp = BloomFilter(ctx, nbytes, k)
    for j, g in enumerate(genomes):
        if j == 0:
            bf.insert(g)
        else:
            tmp.clear()
            tmp.insert(g)
            bf.and_(tmp)
    tmp.free()
    tsvs = [f"{os.path.basename(p)}.k{k}.w{w}.tsv" for p in paths]
    names = [r.names for r in recs]

    def sketch_dev(masks_by_asm, new_w):
        return {i: sketch(ctx, genomes[i], k, new_w, bf, m) for i, m in masks_by_asm.items()}

    plans = []

    def budgeted(eng, budget):
        plain = eng._add

        def add(lists, spans):
            ctx.set_graph_budget(budget)
            try:
                plain(lists, spans)
                plans.append((budget, ctx.graph_last_plan()))
            finally:
                ctx.set_graph_budget(0)
        eng._add = add

    cwd = os.getcwd()
    try:
        engines = []
        for side, budget in (("s", 48 << 10), ("o", 0)):
            os.makedirs(tmp_path / side)
            os.chdir(tmp_path / side)
            eng = DeviceSyntenyEngine(ctx, tsvs, names, k, w, rounds, 10000, 10000, 500, "p", sketch_dev)
            budgeted(eng, budget)
            engines.append(eng)
        a, b = engines
        initial = {i: sketch(ctx, genomes[i], k, w, bf) for i in range(n)}
        handles = [initial[i] for i in a.input_order]
        a._add(handles, None)
        b._add(handles, None)
        for h in handles:
            h.free()
        _states_equal(a, b, "initial add")
        for e in engines:
            e._simplify_dev(apply_deletions=True)
            e._filter(flag=False)
        _states_equal(a, b, "initial filter")
        dbs = [e._blocks() for e in engines]
        prev_w = w
        for new_w in rounds:
            for e, db in zip(engines, dbs):
                masks = e._mask_intervals(db, prev_w)
                lists = e._sketch_round(masks, new_w)
                e._add(lists, e._spans(db))
                for mx in lists:
                    mx.free()
            _states_equal(a, b, f"add w={new_w}")
            last = new_w == rounds[-1]
            for e in engines:
                e._simplify_dev(apply_deletions=False)
                e._filter(flag=last)
                if last:
                    e._erode()
            _states_equal(a, b, f"filter w={new_w}")
            dbs = [e._blocks() for e in engines]
            prev_w = new_w
        assert type(a).rows(dbs[0]) == type(b).rows(dbs[1])
        assert len(type(a).rows(dbs[0])) > 10
    finally:
        os.chdir(cwd)
        for g in genomes:
            g.free()
        bf.free()
    sliced = [p for bud, p in plans if bud]
    assert len(sliced) == 3 and all(p["v_slices"] >= 4 for p in sliced), plans
    assert all(p["v_slices"] == 1 and p["e_slices"] == 1 for bud, p in plans if not bud), plans


def test_an_existing_edge_keeps_its_slot_with_slicing_forced(ctx, tmp_path):
    """nts_engine_add's n_dup path (a new build's edge between vertices that exist, already an edge) with slicing forced on both adds"""
    from ntsynt_amd.device import Minimizers
    from ntsynt_amd.synteny_device import DeviceGraph
    rng = np.random.default_rng(8)
    n = 20000
    hashes = np.unique(rng.integers(1, 1 << 62, size=2 * n, dtype=np.uint64))[:n]
    rng.shuffle(hashes)

    def lists_of(idx, jitter):
        out = []
        for a in range(3):
            pos = (np.arange(idx.size, dtype=np.uint64) * np.uint64(150) + np.uint64(1000 * a + jitter))
            rec = (np.arange(idx.size) >= idx.size // 2).astype(np.uint32)
            out.append((hashes[idx], rec, pos))
        return out
    first = lists_of(np.arange(0, n // 2), 0)
    again = np.sort(rng.choice(np.arange(0, n // 2), size=n // 6, replace=False))
    second = lists_of(np.unique(np.concatenate([np.arange(2000, 5000), again, np.arange(n // 2, n)])), 7)
    graphs = []
    for budget in (32 << 10, 0):
        g = DeviceGraph(ctx, 3, 2)
        ctx.set_graph_budget(budget)
        try:
            for lists in (first, second):
                handles = [Minimizers.from_numpy(ctx, *x) for x in lists]
                g.add(handles)
                for h in handles:
                    h.free()
                if budget:
                    assert ctx.graph_last_plan()["v_slices"] >= 4
        finally:
            ctx.set_graph_budget(0)
        graphs.append(g)
    sa, sb = _engine_state(graphs[0]), _engine_state(graphs[1])
    for f in sa:
        assert np.array_equal(sa[f], sb[f]), f
    assert sa["e_w"].max() >= 3
    for g in graphs:
        g.free()


def test_capacity_sliced_add_peaks_far_below_the_one_pass(tmp_path):
    """Scratch of one nts_engine_add (nts_mem_stats peak over the live bytes before it), each on a fresh context: with the budget an
    eighth of the one-range build's scratch the same add completes, gives the same graph and peaks within the budget plus the arrays
    that stay n- and survivor-sized (docs/design/04_4_graph_stage.md), well under the one-range build."""
    from ntsynt_amd.device import Context, Minimizers
    from ntsynt_amd.synteny_device import DeviceGraph
    rng = np.random.default_rng(11)
    G, n_each = 3, 1_500_000
    core = np.unique(rng.integers(1, 1 << 63, size=n_each + n_each // 4, dtype=np.uint64))
    rng.shuffle(core)
    lists = []
    for a in range(G):
        h = core[:n_each].copy()
        swap = rng.random(n_each) < 0.1                                          # a tenth private to the assembly
        h[swap] = rng.integers(1, 1 << 63, size=int(swap.sum()), dtype=np.uint64)
        rec = (np.arange(n_each) * 4 // n_each).astype(np.uint32)
        lists.append((h, rec, np.arange(n_each, dtype=np.uint64) * np.uint64(40)))
    n = G * n_each
    results, peaks = [], []
    budget = None
    for phase in ("one range", "sliced"):
        c = Context(0)
        try:
            if phase == "sliced":
                c.set_graph_budget(budget)
            handles = [Minimizers.from_numpy(c, *x) for x in lists]
            g = DeviceGraph(c, G, G - 1)
            c.sync()
            c.mem_reset_peak()
            live0 = c.mem_stats()["live"]
            g.add(handles)
            peak = c.mem_stats()["peak"] - live0
            plan = c.graph_last_plan()
            nv, ne = g.size()
            results.append(_engine_state(g))
            peaks.append(peak)
            g.free()
            for h in handles:
                h.free()
        finally:
            c.close()
        if phase == "one range":
            assert plan["v_slices"] == 1
            budget = peak // 8
        else:
            assert plan["v_slices"] >= 2 and plan["e_slices"] >= 2 and plan["oversize"] == 0, plan
    for f in results[0]:
        assert np.array_equal(results[0][f], results[1][f]), f
    m = G * nv
    assert m > n // 2 and ne > nv // 2
    # n-sized: input columns 45 B + vertex ids 4 B + valid mask 1 B; per survivor: columns 12 B, unordered + ordered edges 40 B,
    # vertex results (8 + 12 G) / G B, and the engine's tables and their staging (l2g / rank 20 B per vertex, 37 B per edge)
    bound = budget + 50 * n + (12 + 40 + 12 + 37) * m + (8 + 20 + 3) * nv + 16 * m
    assert peaks[1] <= bound, (peaks, budget, bound)
    assert peaks[1] < 0.75 * peaks[0], peaks


def test_automatic_budget_keeps_the_one_pass(ctx, tmp_path):
    from ntsynt_amd.graph import build_graph_device
    lists = _family_lists(ctx, tmp_path, 3, 45, bp=3_000_000, w=200)
    ctx.set_graph_budget(0)
    build_graph_device(ctx, lists)
    assert ctx.graph_last_plan()["v_slices"] == 1 and ctx.graph_last_plan()["e_slices"] == 1
    assert ctx.graph_last_plan()["oversize"] == 0
    # a build that fits keeps its scratch on the context: the same build again allocates nothing
    live = ctx.mem_stats()["live"]
    build_graph_device(ctx, lists)
    assert ctx.mem_stats()["live"] == live


def test_pipeline_with_graph_budget_writes_the_same_blocks(tmp_path):
    from ntsynt_amd import pipeline
    paths = synth.make_family(str(tmp_path), 3, 2_500_000, 30, 0.01, seed=12, micro=15, n_runs=True, soft_mask=True)
    kw = dict(k=24, w=300, w_rounds=[100, 20], indel=400, merge="10w", block_size=300)
    cwd = os.getcwd()
    out, logs = {}, []
    try:
        for side, budget in (("plain", None), ("sliced", 96 << 10)):
            os.makedirs(tmp_path / side)
            os.chdir(tmp_path / side)
            pipeline.run(paths, prefix="p", log=logs.append, dev=True, graph_budget=budget, **kw)
            out[side] = open("p.synteny_blocks.tsv", "rb").read()
    finally:
        os.chdir(cwd)
    assert len(out["plain"].splitlines()) > 30
    assert out["sliced"] == out["plain"]
    assert any(str(x).startswith("Graph build in slices") for x in logs)

"""Hand-made minimizer lists through the oracle's graph stage, one call at a time (no GPU, no library).

`Brute` drives oracle/synteny_oracle.py step by step -- load, filter_minimizers, build_graph, simplify_graph, filter_graph_global or the
last round's flag + refine_graph, find_paths, blocks_of_paths, split_indels, drop_small(.., 4), and for a later round filter_lists +
build_graph(graph=.., black_list=..) -- and after every step gives the state in the terms ntsynt_amd.synteny_device.DeviceGraph.read
uses: live vertex hashes, live edges as hash pairs with their weights, oriented paths as hash tuples, block rows, the terminal and
internal hash sets and the counters.  The oracle decides; nothing here restates a rule.

Input: lists[a][r] = [(hash, position), ...] of record r of assembly a, in list order (position order in every legal input).  Assembly
a is the engine's index: the oracle sorts file names descending, names() gives assembly a the a-th name of that order, so the last
assembly is the reference (the lexicographically smallest name), as in the engines.

Below it: the shape builders the host and GPU shape tests share.  Each returns lists together with the facts a case must show."""
import numpy as np

from oracle import synteny_oracle as SO


def names(G):
    return [f"g{G - 1 - a:03d}.fa.k24.w100.tsv" for a in range(G)]


def contig(r):
    return f"c{r:05d}"


def tables(records):
    return SO.mx_tables_from_tokens([(contig(r), [(str(int(h)), int(p)) for h, p in rec]) for r, rec in enumerate(records)])


def arrays(records):
    "(h1, rec, pos) of one assembly, as Minimizers.from_numpy takes them"
    h = np.array([x for rec in records for x, _ in rec], np.uint64)
    r = np.array([i for i, rec in enumerate(records) for _ in rec], np.uint32)
    p = np.array([y for rec in records for _, y in rec], np.uint64)
    return h, r, p


class Brute:
    def __init__(self, G, k=24, bp=500, m=90, n=0):
        self.G, self.files = G, names(G)
        self.ora = SO.SyntenyOracle(self.files, {}, k, 100, [], bp, 1000, 0, "x", m=m, n=n)
        assert self.ora.files == self.files
        self.blocks_, self.paths, self.flagged = [], [], []
        self.counts = {"bubbles": 0, "unoriented": 0, "indel_cuts": 0, "small": 0, "eroded": 0}
        self.last = {}                                            # the counters of the last call alone

    # ---- the engine's calls
    def add(self, lists):
        o = self.ora
        if o.graph is None:
            o.load({f: tables(lists[a]) for a, f in enumerate(self.files)})
            o.list_mxs = SO.filter_minimizers(o.list_mxs)
            o.graph = SO.build_graph(o.list_mxs, o.weights)
            return
        assert self.blocks_, "a refinement round without blocks sketches nothing (SyntenyOracle.new_minimizers)"
        new_info, list_mxs = {}, {}
        for a, f in enumerate(self.files):
            new_info[f], list_mxs[f] = tables(lists[a])
        terminal, internal, spans = o.block_marks(self.blocks_)
        filt = SO.filter_minimizers(o.filter_lists(list_mxs, internal, new_info, spans))
        o.update_info(filt, new_info)
        o.graph = SO.build_graph(filt, o.weights, graph=o.graph, black_list=terminal)

    def simplify(self, apply_deletions=True):
        o = self.ora
        g = o.simplify_graph(o.graph)                             # promotes weights in o.graph, deletions in the copy
        if apply_deletions:                                       # (refinement rounds lose the deletions: SyntenyOracle.refine)
            o.graph = g
        self.last = {"bubbles": len(o.last_doomed)}
        self.counts["bubbles"] += len(o.last_doomed)

    def filter(self, flag=False):
        o = self.ora
        light = [e for e in o.graph.edges if e[2] < o.n]
        if flag:
            self.flagged = [(e[0], e[1]) for e in light]
            g = o.graph.copy()
            g.delete_edges([e for e in g.edges if e[2] < o.n])
            o.graph = g
        else:
            o.graph = SO.filter_graph_global(o.graph, o.n, o.weights)
        return len(light)

    def erode(self):
        o = self.ora
        before = len(o.graph.edges)
        o.graph = o.refine_graph(self.flagged)
        self.last = {"eroded": before - len(o.graph.edges)}
        self.counts["eroded"] += self.last["eroded"]

    def blocks(self):
        o = self.ora
        self.paths = SO.find_paths(o.graph, o.list_mx_info[self.files[-1]])
        per_path = [o._blocks_of_path(p) for p in self.paths]
        blocks = [b for bs in per_path for b in bs]
        cut = o.split_indels(blocks)
        kept = o.drop_small(cut, 4)
        self.last = {"unoriented": sum(1 for bs in per_path if not bs), "indel_cuts": len(cut) - len(blocks), "small": len(cut) - len(kept)}
        for key, v in self.last.items():
            self.counts[key] += v
        self.blocks_ = kept

    # ---- the state, in hash terms
    def verts(self):
        return {int(v) for v in self.ora.graph.adj}

    def edges(self):
        return {frozenset((int(e[0]), int(e[1]))): e[2] for e in self.ora.graph.edges}

    def path_tuples(self):
        return sorted(tuple(int(h) for h in p) for p in self.paths)

    def rows(self):
        out = []
        for b in self.blocks_:
            ab = [b.asm[f] for f in self.files]
            out.append((tuple(int(x.contig_id[1:]) for x in ab), tuple(x.ori for x in ab), tuple(x.minimizers[0][1] for x in ab),
                        tuple(x.minimizers[-1][1] for x in ab), b.n_mx()))
        return sorted(out)

    def marks(self):
        terminal, internal, _ = self.ora.block_marks(self.blocks_)
        return {int(h) for h in terminal}, {int(h) for h in internal}

    def degrees(self):
        return {int(v): len(nb) for v, nb in self.ora.graph.adj.items()}

    def components(self):
        "live components as sets of hashes"
        adj, seen, out = self.ora.graph.adj, set(), []
        for v0 in adj:
            if v0 in seen:
                continue
            comp, stack = set(), [v0]
            seen.add(v0)
            while stack:
                v = stack.pop()
                comp.add(int(v))
                for u in adj[v]:
                    if u not in seen:
                        seen.add(u)
                        stack.append(u)
            out.append(comp)
        return out

    def kinds(self):
        "how many components are rings (all degree 2), branching (a degree above 2), isolated vertices"
        deg = self.degrees()
        comps = self.components()
        return {"ring": sum(1 for c in comps if all(deg[v] == 2 for v in c)), "branching": sum(1 for c in comps if any(deg[v] > 2 for v in c)),
                "isolated": sum(1 for c in comps if len(c) == 1)}


# ------------------------------------------------------------------------------------------------------------------------------
# Shape builders.  A Layout collects components; every component takes records of its own in every assembly, so that nothing but
# what the builder wrote joins two vertices.
# ------------------------------------------------------------------------------------------------------------------------------
class Layout:
    def __init__(self, G, seed=0, step=1000):
        self.G, self.rng, self.step = G, np.random.default_rng(seed), step
        self.lists = [[] for _ in range(G)]
        self.used = set()

    def hashes(self, n):
        "n new distinct hashes of 12 to 19 digits, in random order (vertex ids are ranks of hashes: a chain's ids come shuffled)"
        out = []
        while len(out) < n:
            h = int(self.rng.integers(1 << 40, 1 << 62))
            if h not in self.used:
                self.used.add(h)
                out.append(h)
        return out

    def put(self, orders, pos=None):
        """orders[a] = records of the component in assembly a, each a list of hashes in list order; pos[a][hash] = its position
        (default: step, 2 * step, ... along the record).  Returns the record index of each assembly's first record."""
        first = []
        for a in range(self.G):
            first.append(len(self.lists[a]))
            for rec in orders[a]:
                self.lists[a].append([(h, pos[a][h] if pos is not None and h in pos[a] else (i + 1) * self.step) for i, h in enumerate(rec)])
        return first

    # every builder returns the hashes in the order the case speaks of
    def chain(self, n, reverse_in=()):
        "the same n hashes in one record everywhere; in the assemblies of reverse_in the record runs the other way"
        hs = self.hashes(n)
        self.put([[hs[::-1] if a in reverse_in else hs] for a in range(self.G)])
        return hs

    def ring(self, n):
        "assembly 0 lists the ring rotated by one: with the others' chain it closes (every edge has weight below G)"
        hs = self.hashes(n)
        self.put([[hs[1:] + hs[:1] if a == 0 else hs] for a in range(self.G)])
        return hs

    def fork(self, arms):
        "centre c with three arms x, y, z of the given lengths: assembly 0 reads x c z (y apart), the others x c y (z apart)"
        x, y, z = (self.hashes(n) for n in arms)
        c = self.hashes(1)
        self.put([[x[::-1] + c + z, y] if a == 0 else [x[::-1] + c + y, z] for a in range(self.G)])
        return c[0], x, y, z

    def isolated(self):
        h = self.hashes(1)
        self.put([[h] for _ in range(self.G)])
        return h[0]

    def chain_with_changes(self, n, at, asm):
        "chain of n whose record changes before the indices `at` in assembly `asm` (the edge there keeps weight G - 1)"
        hs = self.hashes(n)
        cuts = [0] + sorted(at) + [n]
        self.put([[hs[x:y] for x, y in zip(cuts, cuts[1:])] if a == asm else [hs] for a in range(self.G)])
        return hs

    def bubble(self, mirrored=False, shared=False):
        """a s t b with the bubble s - x - t in the last assembly but one (x apart elsewhere).  shared (G = 4): u between t and b, and
        the last assembly reads a s t u x b -- the edges s - t and t - u both see x as their only common neighbour, and which of
        them still finds its ends partially anchored depends on the promotion made for the other."""
        G = self.G
        if shared:
            assert G == 4
            a, s, t, u, b, x = self.hashes(6)
            orders = [[[a, s, t, u, b], [x]], [[a, s, t, u, b], [x]], [[a, s, x, t, u, b]], [[a, s, t, u, x, b]]]
            out = {"a": a, "s": s, "t": t, "u": u, "b": b, "x": x}
        else:
            a, s, t, b, x = self.hashes(5)
            orders = [[[a, s, x, t, b]] if i == G - 2 else [[a, s, t, b], [x]] for i in range(G)]
            out = {"a": a, "s": s, "t": t, "b": b, "x": x}
        if mirrored:
            orders = [[rec[::-1] for rec in recs] for recs in orders]
        self.put(orders)
        return out

    def two_common(self):
        "G = 4: s - t of full weight, x and y joined to both: a 3-3 edge with two common neighbours, no bubble"
        assert self.G == 4
        s, t, x, y = self.hashes(4)
        self.put([[[x, s, t, y]], [[x, s, t, y]], [[y, s, t, x]], [[y, s, t, x]]])
        return s, t, x, y


def hub(n_asm=150):
    "one hash between a different pair of a 2 * n_asm chain in every assembly: degree 2 * n_asm"
    lay = Layout(n_asm, seed=77)
    xs = lay.hashes(2 * n_asm)
    c = lay.hashes(1)[0]
    lay.put([[xs[:2 * a + 1] + [c] + xs[2 * a + 1:]] for a in range(n_asm)])
    return lay.lists, c, xs


def mixed_run(lay, n_steps, n_up, legal=True):
    """A chain of n_steps + 1 whose positions rise everywhere but in assembly 0, where exactly n_up of the steps along the chain rise.
    legal: assembly 0 lists its record in position order, its stray pairs are edges of weight 1 (needs G >= 3 and n = G - 1 to drop
    them); otherwise assembly 0 keeps the chain's list order with those positions (lists are taken as given: only a refinement round's
    overwritten positions make such a list in a real run)."""
    hs = lay.hashes(n_steps + 1)
    rng = lay.rng
    while True:
        sign = -np.ones(n_steps, np.int64)
        sign[rng.permutation(n_steps)[:n_up]] = 1
        p = np.concatenate(([10 ** 6], 10 ** 6 + np.cumsum(sign * rng.integers(30, 3000, n_steps)))).tolist()
        if len(set(p)) == len(p):
            break
    pos0 = dict(zip(hs, p))
    order0 = sorted(hs, key=pos0.get) if legal else hs
    lay.put([[order0 if a == 0 else hs] for a in range(lay.G)], pos=[pos0 if a == 0 else {} for a in range(lay.G)])
    return hs


def erosion_pair(G, n_s, n_t, s_hash=None, t_hash=None, step_s=1, step_t=1, seed=0, cross=False):
    """Two chains ... c1 s and t d1 ..., adjacent (s t) only in assembly 0: the edge s - t has weight 1 and is flagged.  In the other
    assemblies the two chains lie in records of their own, the i-th vertex from s at 5000 + i * step_s and the i-th from t at
    5003 + i * step_t (default: all within k of each other, so that only the lack of neighbours ends the walk).  cross (G = 3, n = 2): c1 - d1
    joined by an edge of weight 2, so the walk crosses vertices of degree 3."""
    lay = Layout(G, seed=seed)
    cs, ds = lay.hashes(n_s), lay.hashes(n_t)           # cs[0] = s, ds[0] = t
    if s_hash is not None:
        cs[0], ds[0] = s_hash, t_hash
    if cross:
        assert G == 3 and n_s == 3 and n_t == 3
        s, c1, c2, t, d1, d2 = cs[0], cs[1], cs[2], ds[0], ds[1], ds[2]
        left, right = [], []
        near = {h: 1000 + i for i, h in enumerate([c2, c1, d1, d2, s, t])}
        orders = [[left + [c2, c1, s, t, d1, d2] + right], [left + [c2, c1, d1, d2] + right, [s], [t]], [[s, c1, d1, t], [c2], [d2]] + [[h] for h in left + right]]
        lay.put(orders, pos=[{}, near, {}])
        return lay.lists, cs, ds
    pos = {h: 5000 + i * step_s for i, h in enumerate(cs)}
    pos.update({h: 5003 + i * step_t for i, h in enumerate(ds)})
    # (records run in position order: the s chain is listed from s outwards, the t chain as well)
    lay.put([[cs[::-1] + ds] if a == 0 else [cs, ds] for a in range(G)], pos=[{} if a == 0 else pos for a in range(G)])
    return lay.lists, cs, ds


def random_family(seed):
    """A family of 2 to 4 assemblies whose lists are locally perturbed copies of one base order in 1 to 3 records: swaps, reversed
    stretches, record breaks of one assembly alone, dropped hashes, duplicated hashes (which fall out of the filter), a short record
    that one assembly reads rotated (a ring).  Returns (lists, parameters of the run)."""
    rng = np.random.default_rng(1000 + seed)
    G = int(rng.integers(2, 5))
    n_hash = int(rng.integers(30, 201))
    lay = Layout(G, seed=5000 + seed)
    base = lay.hashes(n_hash)
    n_rec = int(rng.integers(1, 4))
    brk = sorted(rng.choice(np.arange(4, n_hash - 4), size=n_rec - 1, replace=False).tolist()) if n_rec > 1 else []
    ringed = n_rec > 1 and rng.random() < 0.5
    if ringed:                                             # the last record is short: one assembly reads it rotated by one
        brk[-1] = n_hash - int(rng.integers(3, 9))
        brk = sorted(set(brk))
    base_recs = [base[x:y] for x, y in zip([0] + brk, brk + [n_hash])]
    dense = rng.random() < 0.5                             # steps below k: erosion has something to walk
    lists = []
    for a in range(G):
        recs = []
        for r, rec in enumerate(base_recs):
            order = list(rec)
            if ringed and r == len(base_recs) - 1:
                recs.append(order[1:] + order[:1] if a == 0 else order)
                continue
            if len(order) < 5:
                recs.append(order)
                continue
            n_ops = max(1, len(order) // 25)
            for _ in range(int(rng.integers(0, n_ops + 1))):   # swaps of neighbours
                i = int(rng.integers(0, len(order) - 1))
                order[i], order[i + 1] = order[i + 1], order[i]
            for _ in range(int(rng.integers(0, n_ops + 1))):   # reversed stretches
                i = int(rng.integers(0, max(1, len(order) - 3)))
                j = i + int(rng.integers(2, 9))
                order[i:j] = order[i:j][::-1]
            if rng.random() < 0.3 and len(order) > 4:          # a dropped hash
                del order[int(rng.integers(0, len(order)))]
            if rng.random() < 0.3:                             # a duplicated hash
                order.insert(int(rng.integers(0, len(order))), order[int(rng.integers(0, len(order)))])
            recs.append(order)
        if len(recs) < 3 and rng.random() < 0.35:              # a record break of this assembly alone
            r = int(rng.integers(0, len(recs) - (1 if ringed else 0))) if len(recs) > (1 if ringed else 0) else 0
            if len(recs[r]) > 6:
                i = int(rng.integers(2, len(recs[r]) - 2))
                recs[r:r + 1] = [recs[r][:i], recs[r][i:]]
        out = []
        for order in recs:
            steps = rng.integers(5, 60, len(order)) if dense else rng.integers(100, 2000, len(order))
            steps = steps + (rng.random(len(order)) < 0.04) * rng.integers(3000, 9000, len(order))   # a gap of this assembly alone: an indel
            out.append(list(zip(order, (np.cumsum(steps) + 1000).tolist())))
        lists.append(out)
    n = 1 if rng.random() < 0.25 else int(rng.integers(max(1, G - 1), G + 1))
    return lists, {"G": G, "k": 24, "bp": 2500, "m": 90, "n": n, "seed": seed}


def refinement_lists(br, seed):
    "a second round for a family: per assembly the block ends again, new hashes before, between and inside the blocks"
    rng = np.random.default_rng(9000 + seed)
    G = br.G
    fresh = Layout(G, seed=9000 + seed).hashes(12)
    term, _ = br.marks()
    out = []
    for a, f in enumerate(br.files):
        info = br.ora.list_mx_info[f]
        recs = {}
        for h in term:
            c, p = info[str(h)]
            recs.setdefault(int(c[1:]), []).append((h, p))
        for i, h in enumerate(fresh):                      # the same new hashes everywhere, next to a block end of the reference order
            th = sorted(term)[i % len(term)]
            c, p = info[str(th)]
            recs[int(c[1:])].append((h, p + int(rng.integers(-40, 41)) + (3 if i % 2 else -3) * 100))
        n_rec = max(recs) + 1
        lst = [[] for _ in range(n_rec)]
        for r, items in recs.items():
            seen, keep = set(), []
            for h, p in sorted(items, key=lambda t: t[1]):
                if p > 0 and p not in seen:
                    seen.add(p)
                    keep.append((h, p))
            lst[r] = keep
        out.append(lst)
    return out

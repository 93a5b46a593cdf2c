"""The hand-made cases of the engine shape tests and the drivers that play them: every case is a script of engine calls over lists from
tests/engine_brute.py's builders, with the facts it must show on the oracle.  Brute (the oracle), Twin (ntsynt_amd/synteny.py fed
arrays directly) and Dev (nts_engine_* through DeviceGraph) answer the same calls and give the same view of their state, in hashes."""
from types import SimpleNamespace

import numpy as np

from tests import engine_brute as EB

BIG = 10 ** 9


# ------------------------------------------------------------------------------------------------------------------------------ drivers
class OracleDriver:
    def __init__(self, G, k=24, bp=500, m=90, n=0):
        self.br = EB.Brute(G, k=k, bp=bp, m=m, n=n)

    def add(self, lists):
        self.br.add(lists)

    def simplify(self, apply_deletions):
        self.br.simplify(apply_deletions)
        return self.br.last["bubbles"]

    def filter(self, flag):
        self.br.filter(flag)

    def erode(self):
        self.br.erode()
        return self.br.last["eroded"]

    def blocks(self):
        br = self.br
        br.blocks()
        terminal, internal = br.marks()
        return {"paths": br.path_tuples(), "rows": br.rows(), "terminal": terminal, "internal": internal, **br.last}

    def graph(self):
        return self.br.verts(), self.br.edges()


class Twin:
    "the host-array engine on arrays: tests/graph_ref.py builds, the native walk, scan and degree helpers do the rest"

    def __init__(self, G, k=24, bp=500, m=90, n=0):
        from ntsynt_amd.graph import edge_degrees, walk_paths
        from ntsynt_amd.synteny import SyntenyEngine
        from tests.graph_ref import build_graph_numpy
        self.e = SyntenyEngine(EB.names(G), [[]] * G, k, 100, [], bp, 1000, 0, "x", build_graph_numpy, None, walk_paths, m=m, n=n,
                               degree_fn=edge_degrees)
        assert self.e.input_order == list(range(G)) and self.e.ref == G - 1
        self.hb, self.flagged = None, (np.zeros(0, np.int64), np.zeros(0, np.int64))

    def add(self, lists):
        arrs = [EB.arrays(x) for x in lists]
        if self.hb is None:
            self.e._add_graph(self.e.graph_fn(arrs, None, None))
        else:
            self.e.sketch_fn = lambda i, masks, w: arrs[i]
            self.e._new_round_graph(self.hb, 10, 100)

    def simplify(self, apply_deletions):
        before = self.e.stats["bubbles"]
        self.e._simplify(apply_deletions)
        return self.e.stats["bubbles"] - before

    def filter(self, flag):
        e = self.e
        light = e.e_alive & (e.e_w < e.n)
        self.flagged = (e.e_u[light], e.e_v[light])
        e.e_alive = e.e_alive & ~light

    def erode(self):
        before = self.e.stats["eroded_edges"]
        self.e._refine_graph(self.flagged)
        return self.e.stats["eroded_edges"] - before

    def blocks(self):
        e = self.e
        before = dict(e.stats)
        verts, off = e._paths()
        paths = sorted(tuple(e.v_hash[verts[off[i]:off[i + 1]]].tolist()) for i in range(off.size - 1))
        hb = e._drop_small(e._blocks_of_paths((verts, off)), 4)
        e._finish_all(hb)
        self.hb = hb
        terminal = {int(e.v_hash[v]) for b in hb for v in (b.vids[0], b.vids[-1])}
        internal = {int(e.v_hash[v]) for b in hb for v in b.vids[1:-1]}
        rows = sorted((tuple(b.rec), tuple(b.ori), tuple(b.first_pos), tuple(b.last_pos), b.n_mx) for b in hb)
        return {"paths": paths, "rows": rows, "terminal": terminal, "internal": internal,
                "unoriented": e.stats["unoriented"] - before["unoriented"], "indel_cuts": e.stats["indel_cuts"] - before["indel_cuts"],
                "small": e.stats["small_blocks"] - before["small_blocks"]}

    def graph(self):
        e = self.e
        vh = e.v_hash
        live = vh[e.v_alive].tolist()
        assert len(set(live)) == len(live)
        m = e.e_alive
        assert e.v_alive[e.e_u[m]].all() and e.v_alive[e.e_v[m]].all()
        return set(live), {frozenset((int(vh[u]), int(vh[v]))): int(w) for u, v, w in zip(e.e_u[m], e.e_v[m], e.e_w[m])}


class Dev:
    "nts_engine_* through DeviceGraph; the bubble rule and the spans of a later round as DeviceSyntenyEngine has them"

    def __init__(self, ctx, G, k=24, bp=500, m=90, n=0):
        from ntsynt_amd.synteny_device import DeviceGraph
        self.ctx, self.G, self.k, self.bp, self.m, self.n = ctx, G, k, bp, m, n or G
        self.g = DeviceGraph(ctx, G, G - 1)
        self.tb = None

    def free(self):
        self.g.free()

    def add(self, lists):
        from ntsynt_amd.device import Minimizers
        from ntsynt_amd.synteny_device import DeviceSyntenyEngine
        spans = DeviceSyntenyEngine._spans(SimpleNamespace(G=self.G), self.tb) if self.tb is not None else None
        handles = []
        try:
            for x in lists:
                handles.append(Minimizers.from_numpy(self.ctx, *EB.arrays(x)))
            self.g.add(handles, spans)
        finally:
            for h in handles:
                h.free()

    def simplify(self, apply_deletions):
        from ntsynt_amd.synteny_device import DeviceSyntenyEngine
        me = SimpleNamespace(graph=self.g, G=self.G, ctx=self.ctx, stats={"bubbles": 0})
        DeviceSyntenyEngine._simplify_dev(me, apply_deletions)
        return me.stats["bubbles"]

    def filter(self, flag):
        self.g.filter(self.n, flag)

    def erode(self):
        return self.g.erode(self.k)

    def blocks(self):
        from ntsynt_amd.synteny_device import DeviceSyntenyEngine
        g = self.g
        tb = g.blocks(self.bp, self.m, 4)
        self.tb = tb
        vh = g.read("v_hash")
        paths = []
        if tb["paths"]:                                       # (no path: the engine holds no path order to read)
            pv, po = g.read("path_verts"), g.read("path_off")
            assert po.size == tb["paths"] + 1 and int(po[-1]) == pv.size
            paths = sorted(tuple(vh[pv[int(po[i]):int(po[i + 1])]].tolist()) for i in range(po.size - 1))
        return {"paths": paths, "rows": DeviceSyntenyEngine.rows(tb), "terminal": set(vh[g.read("terminal").astype(bool)].tolist()),
                "internal": set(vh[g.read("internal").astype(bool)].tolist()), "unoriented": tb["unoriented"],
                "indel_cuts": tb["indel_cuts"], "small": tb["small"]}

    def graph(self):
        g = self.g
        vh, va = g.read("v_hash"), g.read("v_alive").astype(bool)
        live = vh[va].tolist()
        assert len(set(live)) == len(live)
        eu, ev, ew, m = g.read("e_u"), g.read("e_v"), g.read("e_w"), g.read("e_alive").astype(bool)
        assert va[eu[m]].all() and va[ev[m]].all()
        return set(live), {frozenset((int(vh[u]), int(vh[v]))): int(w) for u, v, w in zip(eu[m], ev[m], ew[m])}


def play(driver, script):
    "the script's calls on one driver: [(call, result, (live vertices, live edges)) ...]"
    out = []
    for call in script:
        name, args = call[0], call[1:]
        res = getattr(driver, name)(*args)
        out.append((name, res, driver.graph()))
    return out


def same(want, got, what):
    "state equality after every call: exact"
    assert len(want) == len(got)
    for i, ((name, r0, (v0, e0)), (_, r1, (v1, e1))) in enumerate(zip(want, got)):
        at = f"{what}: call {i} ({name})"
        assert v0 == v1, at + ": live vertices"
        assert e0 == e1, at + ": live edges and weights"
        if isinstance(r0, dict):
            for key in r0:
                assert r0[key] == r1[key], f"{at}: {key}"
        else:
            assert r0 == r1, at + ": count"


# ------------------------------------------------------------------------------------------------------------------------------ cases
# A case: {"G", "par" (k, bp, m, n), "script", "facts": callable(trace of the oracle, its Brute)}.  CASES maps a name to its builder.
FIRST = lambda lists, flag=False: [("add", lists), ("filter", flag), ("blocks",)]                       # noqa: E731
ERODE = lambda lists: [("add", lists), ("filter", True), ("erode",), ("blocks",)]                       # noqa: E731
CHAINS = [2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]


def _lens(trace):
    return sorted(len(p) for p in trace[-1][1]["paths"])


def case_paths():
    lay = EB.Layout(3, seed=1)
    rings = [lay.ring(n) for n in (3, 4, 65)]
    forks = [lay.fork((1, 1, 5)), lay.fork((3, 3, 3))]
    alone = [lay.isolated(), lay.isolated()]
    chains = [lay.chain(n, reverse_in=(2,) if i % 2 else ()) for i, n in enumerate(CHAINS)]

    def facts(trace, br):
        kinds = br.kinds()
        assert kinds == {"ring": 3, "branching": 2, "isolated": 2}
        deg = br.degrees()
        assert all(deg[h] == 2 for r in rings for h in r) and all(deg[f[0]] == 3 for f in forks) and all(deg[h] == 0 for h in alone)
        assert _lens(trace) == CHAINS                       # rings, forks and lone vertices yield no path
        want = sorted(tuple(c[::-1]) if i % 2 else tuple(c) for i, c in enumerate(chains))
        assert trace[-1][1]["paths"] == want                 # a chain the reference reads backwards starts at its other end
    return {"G": 3, "par": dict(bp=BIG, n=1), "script": FIRST(lay.lists), "facts": facts}


def case_hub():
    lists, c, xs = EB.hub(150)

    def facts(trace, br):
        assert br.degrees()[c] == 300 and trace[-1][1]["paths"] == []
    return {"G": 150, "par": dict(bp=BIG, n=1), "script": FIRST(lists), "facts": facts}


def case_long_chain():
    lay = EB.Layout(2, seed=2)
    lay.chain(4097)

    def facts(trace, br):
        assert _lens(trace) == [4097] and trace[-1][1]["rows"][0][4] == 4097
    return {"G": 2, "par": dict(bp=BIG), "script": FIRST(lay.lists), "facts": facts}


def _tie(first_is_smaller):
    "a chain whose two ends lie at the same position of two reference contigs"
    lay = EB.Layout(3, seed=3)
    hs = sorted(lay.hashes(6))
    if not first_is_smaller:
        hs = hs[::-1]
    hs[1:5] = lay.hashes(4)
    ref = {h: p for h, p in zip(hs, (1000, 2000, 3000, 500, 800, 1000))}
    lay.put([[hs[:3], hs[3:]] if a == 2 else [hs] for a in range(3)], pos=[ref if a == 2 else {} for a in range(3)])
    return lay, hs


def case_tie_last_listed_end_is_smaller():
    lay, hs = _tie(False)

    def facts(trace, br):
        info = br.ora.list_mx_info[br.files[-1]]
        assert info[str(hs[0])][1] == info[str(hs[-1])][1] and info[str(hs[0])][0] != info[str(hs[-1])][0]     # the two ends tie
        assert hs[-1] < hs[0] and trace[-1][1]["paths"] == [tuple(hs[::-1])]
    return {"G": 3, "par": dict(bp=BIG, n=2), "script": FIRST(lay.lists), "facts": facts}


def case_contig_changes():
    lay = EB.Layout(3, seed=4)
    plain = lay.chain(12)
    in_ref = lay.chain_with_changes(12, [5], 2)
    in_other = lay.chain_with_changes(12, [7], 0)
    three = lay.chain_with_changes(13, [3, 6, 9], 1)
    at_last = lay.chain_with_changes(9, [8], 0)
    hs = lay.hashes(14)                                       # changes in two assemblies, the later one decides
    lay.put([[hs[:4], hs[4:]], [hs[:9], hs[9:]], [hs]])

    def facts(trace, br):
        res = trace[-1][1]
        assert _lens(trace) == [9, 12, 12, 12, 13, 14]
        assert sorted(r[4] for r in res["rows"]) == [4, 5, 5, 7, 12]       # the last runs: 12, 12 - 5, 12 - 7, 13 - 9, 14 - 9; the run of one is small
        assert res["small"] == 1 and at_last[-1] not in br.verts() and at_last[0] in br.verts()
        assert res["terminal"] >= {three[9], three[12], hs[9], hs[13], in_ref[5], in_other[7], plain[0]}
    return {"G": 3, "par": dict(bp=BIG, n=2), "script": FIRST(lay.lists), "facts": facts}


def case_tiny_paths():
    "2000 paths of 2 and 3 vertices; the paths are numbered by their start vertices, whose hashes rise with the path number here"
    lay = EB.Layout(3, seed=5)
    rng = np.random.default_rng(5)
    lens = [3] * 20 + [2] * 2 + [3] * 64 + rng.integers(2, 4, 2000 - 86).tolist()
    kinds = rng.integers(0, 3, len(lens)).tolist()
    n_mixed = 0
    for i, (n, kind) in enumerate(zip(lens, kinds)):
        hs = [(1 << 39) + i] + lay.hashes(n - 1)
        if kind == 2 and n == 3:                              # assembly 0 has the third between the first two: one step up, one down
            n_mixed += 1
            p0 = {hs[0]: 1000, hs[1]: 3000, hs[2]: 2000}
            lay.put([[[hs[0], hs[2], hs[1]]] if a == 0 else [hs] for a in range(3)], pos=[p0, {}, {}])
        else:
            lay.put([[hs[::-1] if (a == 0 and kind == 1) else hs] for a in range(3)])
    off = np.concatenate(([0], np.cumsum(lens)))

    def facts(trace, br):
        res = trace[-1][1]
        assert [len(p) for p in sorted(res["paths"])] == lens and {64, 256} <= set(off.tolist())   # boundaries at lanes 63/64 and 255/256
        assert res["unoriented"] == n_mixed > 300 and res["small"] == len(lens) - n_mixed and res["rows"] == []
    return {"G": 3, "par": dict(bp=BIG, n=2), "script": FIRST(lay.lists), "facts": facts}


STEPS = [(10, 9), (10, 1), (100, 90), (100, 89), (100, 11), (100, 10), (10, 5), (10, 4), (10, 6), (1, 1), (1, 0), (3, 3), (3, 0), (20, 10)]


def _orientation(G, m):
    def build():
        lay = EB.Layout(G, seed=10 * G + m)
        for n_steps, n_up in STEPS:
            EB.mixed_run(lay, n_steps, n_up, legal=G > 2)
        want = []
        for n_steps, n_up in STEPS:                           # synteny_block.py:48-65 in whole numbers: up / n * 100 >= m
            code = "+" if n_up == n_steps else "-" if n_up == 0 else "+" if n_up * 100 >= m * n_steps else \
                "-" if (n_steps - n_up) * 100 >= m * n_steps else "?"
            want.append((code, n_steps + 1))

        def facts(trace, br):
            res = trace[-1][1]
            assert res["unoriented"] == sum(1 for c, _ in want if c == "?") and (res["unoriented"] > 0 or m == 50)
            assert sorted((r[1][0], r[4]) for r in res["rows"]) == sorted((c, n) for c, n in want if c != "?" and n >= 4)
            assert all(set(r[1][1:]) == {"+"} for r in res["rows"])           # mixed in assembly 0 only
        return {"G": G, "par": dict(bp=BIG, m=m, n=max(G - 1, 2)), "script": FIRST(lay.lists), "facts": facts}
    return build


def case_indel_cuts():
    lay = EB.Layout(3, seed=6)
    a = lay.hashes(12)                                        # gaps of assembly 0 over the threshold by one after 3 and after 7: pieces of 3, 4, 5
    pa = {h: 1000 * (i + 1) + 501 * ((i >= 3) + (i >= 7)) for i, h in enumerate(a)}
    lay.put([[a]] * 3, pos=[pa, {}, {}])
    b = lay.hashes(6)                                         # exactly the threshold: no cut
    pb = {h: 1000 * (i + 1) + 500 * (i >= 3) for i, h in enumerate(b)}
    lay.put([[b]] * 3, pos=[{}, pb, {}])

    def facts(trace, br):
        res = trace[-1][1]
        assert res["indel_cuts"] == 2 and res["small"] == 1 and sorted(r[4] for r in res["rows"]) == [4, 5, 6]
        edges = br.edges()
        assert frozenset((a[2], a[3])) not in edges and frozenset((a[6], a[7])) not in edges and frozenset((b[2], b[3])) in edges
        assert not {a[0], a[1], a[2]} & br.verts()
    return {"G": 3, "par": dict(bp=500), "script": FIRST(lay.lists), "facts": facts}


def _weight_filter(n):
    def build():
        lay = EB.Layout(3, seed=7)
        hs = lay.chain_with_changes(10, [5], 0)               # one edge of weight G - 1

        def facts(trace, br):
            assert trace[0][2][1][frozenset((hs[4], hs[5]))] == 2
            assert _lens(trace) == ([5, 5] if n == 3 else [10])
        return {"G": 3, "par": dict(bp=BIG, n=n), "script": FIRST(lay.lists), "facts": facts}
    return build


def _erosion(kind):
    def build():
        G, n = 2, 2
        if kind in ("9_10", "10_9", "19_20", "20_19"):
            lo, hi = (9, 10) if "9" == kind[0] or kind == "10_9" else (9999999999999999999, 10000000000000000000)
            s, t = (lo, hi) if kind in ("9_10", "19_20") else (hi, lo)
            lists, cs, ds = EB.erosion_pair(2, 4, 4, s_hash=s, t_hash=t, step_t=30)
        elif kind == "long":
            lists, cs, ds = EB.erosion_pair(2, 60, 60, seed=1)
        elif kind == "short":
            lists, cs, ds = EB.erosion_pair(2, 2, 3, seed=2)
        elif kind == "distance":
            lists, cs, ds = EB.erosion_pair(2, 8, 8, step_t=10, seed=3)
        elif kind == "cross":
            G = 3
            lists, cs, ds = EB.erosion_pair(3, 3, 3, cross=True, seed=4)
        else:                                                 # "inner": the flagged edge leaves the middle of a chain
            G = 3
            lay = EB.Layout(3, seed=5)
            x, d = lay.hashes(5), lay.hashes(3)
            lay.put([[x, d], [x, d], [x[:3] + d, x[3:]]])
            lists, cs, ds = lay.lists, x, d

        def facts(trace, br):
            eroded, after = trace[2][1], trace[2][2][1]
            before = trace[1][2][1]
            gone = set(before) - set(after)
            assert len(gone) == eroded
            if kind in ("9_10", "10_9", "19_20", "20_19"):    # the greater NAME is the target and is eroded first
                target = max(cs[0], ds[0], key=str)
                assert min(cs[0], ds[0], key=str) == max(cs[0], ds[0]) and any(target in e for e in gone)
                # the t chain is spread out: as the target it ends the walk after one step, as the source after the target's first
                assert eroded == (1 if target == ds[0] else 2)
            elif kind == "long":
                assert eroded == 118 and not after            # the walk visits all 120 vertices: more than the kernel's 96
            elif kind == "short":
                assert eroded == 3 and not after              # both chains to their ends: the walk runs out of neighbours
            elif kind == "distance":
                assert 0 < eroded < 14 and any(cs[0] in e for e in gone) and any(ds[0] in e for e in gone)     # both sides in turn
            elif kind == "cross":
                assert max(br_deg for br_deg in trace_deg(before).values()) == 3 and eroded == 5 and not after
            else:
                assert eroded == 0 and trace_deg(before)[cs[2]] == 2
        return {"G": G, "par": dict(bp=BIG, n=n), "script": ERODE(lists), "facts": facts}
    return build


def trace_deg(edges):
    deg = {}
    for e in edges:
        for v in e:
            deg[v] = deg.get(v, 0) + 1
    return deg


def _bubbles(shape, apply_deletions):
    def build():
        G = 3 if shape in ("one", "one_mirrored") else 4
        lay = EB.Layout(G, seed=8)
        lay.chain(6)
        if shape == "two_common":
            s, t, x, y = lay.two_common()
            b = {"x": x, "s": s, "t": t}
        else:
            b = lay.bubble(mirrored=shape.endswith("mirrored"), shared=shape.startswith("shared"))
        script = [("add", lay.lists), ("simplify", apply_deletions), ("filter", False), ("blocks",)]

        def facts(trace, br):
            n_found = trace[1][1]
            deg0 = trace_deg(trace[0][2][1])
            assert deg0[b["s"]] == 3 and deg0[b["t"]] == 3
            # shared: s - t is promoted first, after which t - u no longer has a partially anchored end; mirrored, t - u comes first and both fire
            assert n_found == {"one": 1, "one_mirrored": 1, "shared": 1, "shared_mirrored": 2, "two_common": 0}[shape]
            if shape != "two_common":
                assert (b["x"] in trace[1][2][0]) == (not apply_deletions)
                assert trace[1][2][1][frozenset((b["s"], b["t"]))] == G
                # the deletion turns the branching component into a path; without it the component yields none
                assert _lens(trace) == ([4 + shape.startswith("shared"), 6] if apply_deletions else [6])
        return {"G": G, "par": dict(bp=BIG, n=1), "script": script, "facts": facts}
    return build


def _second_add(where):
    def build():
        lay = EB.Layout(2, seed=9)
        hs = lay.hashes(6)
        lay.put([[hs], [hs]], pos=[{h: 1000 * (i + 1) + 7 for i, h in enumerate(hs)}, {}])
        y0, y1, x = lay.hashes(3)
        lo, hi = 1000, 6000                                    # the block's interior is [lo + 1, hi)
        p = {"lo": lo, "start": lo + 1, "inside": lo + 2, "last_inside": hi - 1, "end_max": hi}[where]
        second = []
        for a in range(2):
            d = 7 if a == 0 else 0
            second.append([sorted([(y0, lo - 500 + d), (hs[0], lo + d), (x, p + d), (hs[5], hi + d), (y1, hi + 500 + d)], key=lambda t: (t[1], (t[0] == x) == (where == "lo")))])   # (x shares its position with a block end at lo and end_max: it is listed on the inner side)
        script = [("add", lay.lists), ("filter", False), ("blocks",), ("add", second), ("simplify", False), ("filter", False), ("blocks",)]

        def facts(trace, br):
            assert trace[2][1]["terminal"] == {hs[0], hs[5]} and trace[2][1]["internal"] == set(hs[1:5])
            verts, edges = trace[3][2]
            assert (x in verts) == (where in ("lo", "end_max")) and {y0, y1} <= verts
            # the block ends are vertices already and take the new edges; the list is cut where it crosses the interior
            assert frozenset((y0, hs[0])) in edges and frozenset((hs[5], y1)) in edges
            assert not any(frozenset((u, v)) in edges for u in (hs[0], x) for v in (hs[5], x) if u != v and {u, v} != {hs[0], x} and {u, v} != {x, hs[5]})
        return {"G": 2, "par": dict(bp=BIG), "script": script, "facts": facts}
    return build


CASES = {"paths": case_paths, "hub": case_hub, "long_chain": case_long_chain, "tie": case_tie_last_listed_end_is_smaller,
         "contig_changes": case_contig_changes, "tiny_paths": case_tiny_paths, "indel_cuts": case_indel_cuts,
         "weight_filter_n3": _weight_filter(3), "weight_filter_n2": _weight_filter(2)}
CASES.update({f"orientation_G{G}_m{m}": _orientation(G, m) for G in (2, 3, 9) for m in (90, 50)})
CASES.update({f"erosion_{kind}": _erosion(kind) for kind in ("9_10", "10_9", "19_20", "20_19", "long", "short", "distance", "cross", "inner")})
CASES.update({f"bubbles_{shape}_{'applied' if ap else 'kept'}": _bubbles(shape, ap)
              for shape in ("one", "one_mirrored", "shared", "shared_mirrored", "two_common") for ap in (True, False)})
CASES.update({f"second_add_{where}": _second_add(where) for where in ("lo", "start", "inside", "last_inside", "end_max")})


def oracle_trace(case):
    d = OracleDriver(case["G"], **case["par"])
    return play(d, case["script"]), d.br


def random_script(seed):
    "the first-round sequence of a family (every fifth: one refinement add on top), as a case"
    lists, par = EB.random_family(seed)
    return {"G": par["G"], "par": dict(k=par["k"], bp=par["bp"], m=par["m"], n=par["n"]),
            "script": [("add", lists), ("simplify", True), ("filter", True), ("erode",), ("blocks",)], "refine": seed % 5 == 0, "seed": seed}


REFINE = [("simplify", False), ("filter", True), ("erode",), ("blocks",)]

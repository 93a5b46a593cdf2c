"""nts_sketch_ex at the places where its kernels are built to differ: the seams of their tiles, the window limit, and the masks of a
refinement round in every shape build_runs has to sort, merge and clip -- every way a sketch can go, against the oracle, exactly.

The inputs are constructed (tests/sketch_cases.py; tests/test_sketch_cases_host.py checks on the CPU that they hold what is relied on
here): a genome whose runs end, begin and tie on m T - 1, m T and m T + 1 for every tile size T the ways cut the compact k-mer index by,
a filter that leaves a window uncovered across such a seam, and mask lists that overlap, nest, repeat, abut N runs and record ends.
Every expectation is oracle_flat(O.minimize(...)); h1, rec and pos are compared with np.array_equal: the sketch is exact.  After each
call the counters say which way ran, and every cell prints its way, (k, w), the filter's accepted share, the minimizers and the
uncovered ranges.  Every test runs under a time limit of its own (a hung call ends the process, with a traceback).  Needs an MI355X."""
import faulthandler

import numpy as np
import pytest

from oracle import nts_oracle as O
from tests import sketch_cases as SC
from tests.helpers import oracle_flat, to_device, to_oracle

pytestmark = pytest.mark.gpu
STEP_SECONDS = 600
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
TIMERS = ("hash_tiers", "hash_accept", "hash_select", "hash_select_nofilter", "sparse_win", "window_min", "hash_probe", "hash_only")


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


def same(got, exp, what):
    for name, a, b in zip(("h1", "rec", "pos"), got, exp):
        b = b.astype(a.dtype)
        if not np.array_equal(a, b):
            n = min(a.size, b.size)
            at = int(np.flatnonzero(a[:n] != b[:n])[0]) if (a[:n] != b[:n]).any() else n
            first = [(int(x[1][at]), int(x[2][at])) if at < x[0].size else None for x in (got, exp)]
            raise AssertionError(f"{what}: {name} differs from the oracle at element {at} of {a.size} / {b.size}: (rec, pos) got {first[0]}, expected {first[1]}")


def reset(c):
    c.sketch_mode("auto", 0)
    c.sketch_select("auto")
    c.sketch_tiers("auto")
    c.sketch_summary("auto")
    c.profile(0)


def relative(rng, seqs, rate):
    out = []
    for s in seqs:
        a = np.frombuffer(s, dtype=np.uint8).copy()
        hit = (rng.random(a.size) < rate) & (a != ord("N"))
        a[hit] = ACGT[rng.integers(0, 4, size=int(hit.sum()))]
        out.append(a.tobytes())
    return out


_genomes = {}


def seam_case(k, w):
    "the seam genome of (k, w) with its oracle container, hashes, filters and expected lists: built once, left unchanged"
    if (k, w) not in _genomes:
        if len(_genomes) > 2:
            _genomes.clear()
        names, seqs, placed = SC.seam_genome(k, w)
        missing = SC.expected_properties(w) - {(p, T, d) for p, T, d, _ in placed}
        assert not missing, sorted(missing)
        og = to_oracle(names, seqs)
        _genomes[(k, w)] = dict(names=names, seqs=seqs, placed=placed, og=og, h0=SC.hashes(og, k), filters={}, exp={},
                                nbytes=O.bf_ctor_bytes(O.bf_approx_bytes(og.total_bp, 0.04)))     # (4 % of the bits set: too full for a summary, plan_sketch: `sum_max`)
    return _genomes[(k, w)]


def case_filter(case, k, kind):
    "kind: None, 'seam', 'sparse' (the seam filter over one k-mer in sixteen), 'out' (the seam filter and a filter-out filter)"
    if kind not in case["filters"]:
        common = repeat = None
        if kind is not None:
            common = SC.seam_filter(case["og"], k, case["nbytes"], case["placed"], keep=16 if kind == "sparse" else 1)
        if kind == "out":
            repeat = O.repeat_bf([case["og"]], k, 40000)          # the k-mers seen twice: the homopolymers and the AC repeats on the seams
            assert O.bf_popcount(repeat) > 0
        case["filters"][kind] = (common, repeat)
    return case["filters"][kind]


def expected(case, k, w, kind):
    if kind not in case["exp"]:
        common, repeat = case_filter(case, k, kind)
        case["exp"][kind] = oracle_flat(O.minimize(case["og"], k, w, common, repeat=repeat))
    return case["exp"][kind]


def run_cell(c, way, k, w, kind, setup, check, env=None):
    """One cell: the seam genome of (k, w) through `way` with filter `kind`; setup(c) switches the way on, check(c, counts, stats)
    asserts from the counters that it ran."""
    from ntsynt_amd.device import BloomFilter, sketch
    case = seam_case(k, w)
    common, repeat = case_filter(case, k, kind)
    exp = expected(case, k, w, kind)
    dg = to_device(c, case["names"], case["seqs"])
    dbf = drep = None
    try:
        if common is not None:
            dbf = BloomFilter(c, common.size, k)
            dbf.from_numpy(common)
        if repeat is not None:
            drep = BloomFilter(c, repeat.size, k)
            drep.from_numpy(repeat)
        setup(c)
        c.profile(1)
        mx = sketch(c, dg, k, w, dbf, None, repeat=drep)
        got = mx.to_numpy()
        c.sync()
        counts = {t: c.timing(t)[1] for t in TIMERS}
        stats = dict(zip(("candidates", "uncovered_ranges", "uncovered_kmers"), c.sketch_stats()))
        stats["tiers"] = c.sketch_tiers()[2]
        stats["summary_shift"] = c.sketch_summary()
        share = float(SC.accepted(common, case["h0"]).mean()) if common is not None else 1.0
        print(f"way={way} k={k} w={w} filter={kind} accepted={share:.3f} minimizers={got[0].size} uncovered_ranges={stats['uncovered_ranges']} "
              f"candidates={stats['candidates']} tiers={stats['tiers']} summary_shift={stats['summary_shift']} "
              f"launches={ {t: n for t, n in counts.items() if n} } bases={case['og'].total_bp}{' ' + str(env) if env else ''}")
        assert exp[0].size > 50
        same(got, exp, f"{way} k={k} w={w} filter={kind}")
        check(c, counts, stats)
        mx.free()
    finally:
        reset(c)
        for x in (dbf, drep, dg):
            if x is not None:
                x.free()
    return stats


# ---- 1. every way over the seams -------------------------------------------------------------------------------------------------------
def ran_dense(k, w, kind):
    def check(c, n, st):
        # every k-mer probed: no candidate list, no tiers, no accept list; the window tiles hash their own k-mers below w = 64
        # (k_window_min<true>, timed as the hashing pass) unless k > FAST_K_MAX, else the key array and k_window_min<false>
        assert (st["candidates"], st["uncovered_ranges"], st["uncovered_kmers"]) == (0, 0, 0) and st["tiers"] == 0, st
        assert n["hash_tiers"] == n["hash_accept"] == n["sparse_win"] == n["hash_select"] == n["hash_select_nofilter"] == 0, n
        assert n["hash_probe"] + n["hash_only"] >= 1, n
        if w >= 64 or k > 128:
            assert n["window_min"] >= 1, n
        elif st["summary_shift"] == 0:
            assert n["window_min"] == 0, n
    return check


def ran_one_threshold(kind):
    def check(c, n, st):
        assert st["candidates"] > 0 and st["tiers"] == 0, st
        assert n["hash_select" if kind else "hash_select_nofilter"] >= 1 and n["sparse_win"] >= 1 and n["hash_tiers"] == n["hash_accept"] == 0, n
        if kind:
            assert st["uncovered_ranges"] > 0, "the seam filter's rejected stretch left no window uncovered"
    return check


def ran_tiers(c, n, st):
    assert st["tiers"] >= 2 and n["hash_tiers"] >= 1 and n["sparse_win"] >= 1, (st, n)
    assert st["uncovered_ranges"] == 0 and n["hash_accept"] == n["hash_select"] == n["hash_select_nofilter"] == 0, (st, n)


def ran_accept_list(c, n, st):
    assert st["summary_shift"] >= 7 and n["hash_accept"] >= 1 and n["sparse_win"] >= 1, (st, n)
    assert st["uncovered_ranges"] == 0 and n["hash_tiers"] == n["hash_select"] == 0, (st, n)


# dense: sketch mode "dense" is Dense for every (k, w) (plan_sketch: `pruned` is false, the tiers ask for sketch mode "auto")
DENSE = [(24, 10), (24, 63), (24, 64), (24, 250)]


def cells(grid, kinds, out_cell):
    "every (k, w) with every filter kind, and the filter-out filter for one cell of the way"
    return [(k, w, kind) for k, w in grid for kind in kinds] + [(*out_cell, "out")]


@pytest.mark.parametrize("k,w,kind", cells(DENSE, (None, "seam"), (24, 64)))
def test_dense_over_the_seams(ctx, k, w, kind):
    run_cell(ctx, "dense", k, w, kind, lambda c: c.sketch_mode("dense"), ran_dense(k, w, kind))


# one threshold: sketch mode "pruned" keeps `pruned` whatever w (plan_sketch: `pruned = ctx->sketch_mode == 2`), the tiers are not looked at;
# run_pruned takes k_hash_select_hi for k <= 32 when told to ("hi": these genomes are in pieces, left alone it keeps k_hash_select), with
# two listed k-mers per lane and round at (24, 1000) and (32, 1000) and four at (24, 250) (4096 c / w against 128 / 1.2); k = 40 is beyond
# the upper-halves kernel in every setting.  A filter-out filter turns the call Dense (`if (filter_out) pruned = false`).
PRUNED_HI = [(24, 250), (24, 1000), (32, 1000)]


@pytest.mark.parametrize("k,w,kind", cells(PRUNED_HI, (None, "seam"), (24, 1000)))
def test_one_threshold_upper_halves_over_the_seams(ctx, k, w, kind):
    if kind == "out":
        run_cell(ctx, "pruned+filter-out", k, w, kind, lambda c: c.sketch_mode("pruned"), ran_dense(k, w, kind))
        return

    def hi(c):
        c.sketch_mode("pruned")
        c.sketch_select("hi")

    def full(c):
        c.sketch_mode("pruned")
        c.sketch_select("full")
    st_hi = run_cell(ctx, "pruned select=hi", k, w, kind, hi, ran_one_threshold(kind))
    st_full = run_cell(ctx, "pruned select=full", k, w, kind, full, ran_one_threshold(kind))
    # the upper-halves kernel drops the accepted k-mers that cannot win a window where a tile lies in one run, the full-width one lists
    # them all: fewer candidates is how the counters tell the two apart
    assert st_hi["candidates"] < st_full["candidates"], (st_hi, st_full)


@pytest.mark.parametrize("tpw", ["1", "3"])
@pytest.mark.parametrize("kind", [None, "seam"])
@pytest.mark.parametrize("k,w", PRUNED_HI)
def test_one_threshold_upper_halves_tiles_per_wave(ctx_x, monkeypatch, k, w, kind, tpw):
    "the same on the experiments build with one and three wave tiles per wave (NTS_HI_TPW): a wave's second tile begins on a seam of 4096"
    monkeypatch.setenv("NTS_HI_TPW", tpw)

    def hi(c):
        c.sketch_mode("pruned")
        c.sketch_select("hi")
    run_cell(ctx_x, "pruned select=hi", k, w, kind, hi, ran_one_threshold(kind), env=f"NTS_HI_TPW={tpw}")


@pytest.mark.parametrize("kind", [None, "seam"])
def test_one_threshold_full_width_over_the_seams(ctx, kind):
    k, w = 40, 1000                                               # k > HI_K_MAX = 32: run_pruned's `sel_hi` is false whatever is asked for

    def any_select(c):
        c.sketch_mode("pruned")
        c.sketch_select("hi")
    st_a = run_cell(ctx, "pruned k>32 select=hi", k, w, kind, any_select, ran_one_threshold(kind))

    def full(c):
        c.sketch_mode("pruned")
        c.sketch_select("full")
    st_b = run_cell(ctx, "pruned k>32 select=full", k, w, kind, full, ran_one_threshold(kind))
    assert st_a["candidates"] == st_b["candidates"]              # one kernel both times


# tiers forced: plan_sketch takes them for k <= FAST_K_MAX = 128, 8 <= w <= 4097 and c0 = x0 / p <= w / 2 (`tiers_forced`, then the block
# under "Tiered selection": `ctx->tier_mode == 2` passes `pays` and the comparison with the one threshold); no summary in front of them
TIERS = [(24, 10), (24, 63), (24, 64), (24, 250), (24, 1000), (24, 4097)]


@pytest.mark.parametrize("k,w,kind", cells(TIERS, (None, "seam"), (24, 250)))
def test_tiers_over_the_seams(ctx, k, w, kind):
    if kind == "out":                                             # (`tiers_forced` asks for no filter-out filter: the call is Dense)
        run_cell(ctx, "tiers+filter-out", k, w, kind, lambda c: c.sketch_tiers("always"), ran_dense(k, w, kind))
        return
    run_cell(ctx, "tiers", k, w, kind, lambda c: c.sketch_tiers("always"), ran_tiers)


# accept list: a filter that holds one k-mer in sixteen sets 0.2 of its summary's bits (below 0.7 against the tiers, 3.0 against Dense:
# plan_sketch's `sum_max`), sketch mode "auto" then lists the accepted k-mers (`plan.sel = SketchSel::AcceptList`)
ACCEPT = [(24, 100), (24, 1000)]


def no_accept_list(c, n, st):
    assert n["hash_accept"] == 0 and st["summary_shift"] == 0, (st, n)


@pytest.mark.parametrize("k,w,kind", cells(ACCEPT, (None, "sparse"), (24, 100)))
def test_accept_list_over_the_seams(ctx, k, w, kind):
    if kind == "sparse":
        run_cell(ctx, "accept list", k, w, kind, lambda c: c.sketch_summary("auto"), ran_accept_list)
    elif kind is None:                                            # without a filter there is nothing to list: the automatic choice, against the oracle
        run_cell(ctx, "auto (no filter)", k, w, kind, lambda c: c.sketch_summary("auto"), no_accept_list)
    else:
        run_cell(ctx, "auto+filter-out", k, w, kind, lambda c: c.sketch_summary("auto"), ran_dense(k, w, kind))


@pytest.mark.parametrize("kind", [None, "seam", "out"])
def test_run_table_walk_over_the_seams(ctx, kind):
    "k = 129 > FAST_K_MAX: no LDS staging, every tile walks the run table (k_hash's generic walk and the window kernel), the tiers do not apply"
    run_cell(ctx, "run-table walk", 129, 50, kind, lambda c: None, ran_dense(129, 50, kind))


# ---- 2. large windows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [4097, 4098, 8191, 8192, 11999, 12000])
def test_large_windows(ctx, w):
    """Above the tiers' last window and up to WIN_MAX_W = 12000, where k_window_min asks for (WIN_TILE + w) * 8 bytes and its tables of
    LDS: no filter, a filter that accepts about 70 % (a relative at 2 %, as test_sketch_with_filter builds it) and the seam filter, whose
    uncovered windows go through the window kernel here (the tiers that take them below end at 4097), under auto, dense and pruned."""
    from ntsynt_amd.device import BloomFilter, sketch
    k = 24
    case = seam_case(k, w)
    og, names, seqs = case["og"], case["names"], case["seqs"]
    rng = np.random.default_rng(w)
    other = to_oracle(names, relative(rng, seqs, 0.02))
    obf = O.bf_build(other, k, case["nbytes"], prev=O.bf_build(og, k, case["nbytes"]))
    share = float(SC.accepted(obf, case["h0"]).mean())
    assert 0.6 < share < 0.8, share
    dg = to_device(ctx, names, seqs)
    dbf = BloomFilter(ctx, obf.size, k)
    dbf.from_numpy(obf)
    try:
        seam = case_filter(case, k, "seam")[0]
        sbf = BloomFilter(ctx, seam.size, k)
        sbf.from_numpy(seam)
        for label, bf_o, bf_d, acc in ((None, None, None, 1.0), ("70%", obf, dbf, share), ("seam", seam, sbf, float(SC.accepted(seam, case["h0"]).mean()))):
            exp = oracle_flat(O.minimize(og, k, w, bf_o))
            assert exp[0].size > 20
            for mode in ("auto", "dense", "pruned"):
                ctx.sketch_mode(mode)
                ctx.profile(1)
                got = sketch(ctx, dg, k, w, bf_d).to_numpy()
                ctx.sync()
                cand, ranges, range_kmers = ctx.sketch_stats()
                print(f"way={mode} k={k} w={w} filter={label} accepted={acc:.3f} minimizers={got[0].size} "
                      f"uncovered_ranges={ranges} candidates={cand} window_min={ctx.timing('window_min')[1]} bases={og.total_bp}")
                same(got, exp, f"{mode} k={k} w={w} filter={label}")
                assert ctx.sketch_tiers()[2] == 0                 # (the tiers end at 4097 and are not asked for)
                if mode == "dense":
                    assert (cand, ranges, range_kmers) == (0, 0, 0) and ctx.timing("window_min")[1] >= 1
                if mode == "pruned":
                    assert cand > 0
                    if label == "seam":
                        assert ranges > 0 and ctx.timing("window_min")[1] >= 1, "the seam filter's rejected stretch left no window uncovered"
        sbf.free()
    finally:
        reset(ctx)
        dbf.free()
        dg.free()


def test_the_window_limit_on_either_side(ctx):
    "w = 12001 is refused with NTS_ERANGE; the next call at 12000 on the same context and genome gives the oracle's list"
    from ntsynt_amd.device import NtsError, sketch
    k = 24
    case = seam_case(k, 12000)
    dg = to_device(ctx, case["names"], case["seqs"])
    try:
        for mode in ("auto", "dense", "pruned"):
            ctx.sketch_mode(mode)
            with pytest.raises(NtsError, match=r"\(code -34\)"):                 # NTS_ERANGE
                sketch(ctx, dg, k, 12001)
            same(sketch(ctx, dg, k, 12000).to_numpy(), expected(case, k, 12000, None), f"w = 12000 after the refusal, {mode}")
    finally:
        reset(ctx)
        dg.free()


def test_the_largest_window_on_records_too_short_for_it(ctx):
    "w = 12000 on a genome whose every record has fewer than w valid k-mers: an empty list, no error"
    from ntsynt_amd.device import sketch
    from tests.helpers import random_records
    k, w = 24, 12000
    rng = np.random.default_rng(12)
    seqs = random_records(rng, [w + k - 2, 0, 11000, w + k - 2, 5, 12100, 8192 + k - 1], n_frac=0.0, lower_frac=0.02)
    last = bytearray(seqs[5])
    for at in (2000, 4000, 6000, 8000, 10000):                     # 12100 bases with five N: k-mers enough by length, not by count
        last[at] = ord("N")
    seqs[5] = bytes(last)
    names = [f"r{i}" for i in range(len(seqs))]
    lay = SC.Layout(seqs, k)
    assert lay.rec_nv.max() == w - 1 and (np.array([len(s) for s in seqs]) - k + 1).max() >= w
    assert oracle_flat(O.minimize(to_oracle(names, seqs), k, w))[0].size == 0
    dg = to_device(ctx, names, seqs)
    try:
        for mode in ("auto", "dense", "pruned"):
            ctx.sketch_mode(mode)
            got = sketch(ctx, dg, k, w).to_numpy()
            assert [a.size for a in got] == [0, 0, 0], mode
    finally:
        reset(ctx)
        dg.free()


# ---- 3. masks equal N-substitution -----------------------------------------------------------------------------------------------------
_mask_cases = {}


def mask_case(k):
    if k not in _mask_cases:
        rng = np.random.default_rng(700 + k)
        names, seqs, n_runs = SC.mask_family(k, rng)
        sets = list(SC.mask_sets([len(s) for s in seqs], k, rng, n_runs))
        og = to_oracle(names, seqs)
        nbytes = O.bf_ctor_bytes(O.bf_approx_bytes(og.total_bp, 0.3))
        obf = O.bf_build(og, k, nbytes)
        obf[::3] = 0                                               # holes: the filter rejects a third of the k-mers everywhere
        _mask_cases[k] = dict(names=names, seqs=seqs, sets=sets, og=og, obf=obf, masked={}, exp={})
    return _mask_cases[k]


def masks_equal_substitution(c, k, w, setup, way, went=lambda c: True):
    from ntsynt_amd.device import BloomFilter, sketch
    case = mask_case(k)
    names, seqs = case["names"], case["seqs"]
    dg = to_device(c, names, seqs)
    dbf = BloomFilter(c, case["obf"].size, k)
    dbf.from_numpy(case["obf"])
    share = float(SC.accepted(case["obf"], SC.hashes(case["og"], k)).mean())
    try:
        for bf_o, bf_d in ((None, None), (case["obf"], dbf)):
            for name, masks in case["sets"]:
                if name not in case["masked"]:
                    case["masked"][name] = SC.apply_masks(seqs, masks)
                masked = case["masked"][name]
                key = (name, w, bf_o is not None)
                if key not in case["exp"]:
                    case["exp"][key] = oracle_flat(O.minimize(to_oracle(names, masked), k, w, bf_o))
                exp = case["exp"][key]
                setup(c)
                got = sketch(c, dg, k, w, bf_d, masks).to_numpy()
                ranges = c.sketch_stats()[1]
                assert got[0].size == 0 or went(c), f"masks '{name}' k={k} w={w}: the call did not go the way {way}"
                dm = to_device(c, names, masked)
                sub = sketch(c, dm, k, w, bf_d).to_numpy()
                dm.free()
                print(f"way={way} k={k} w={w} masks='{name}' ({len(masks)}) filter={bf_o is not None} accepted={share if bf_o is not None else 1.0:.3f} "
                      f"minimizers={got[0].size} uncovered_ranges={ranges}")
                same(got, exp, f"masks '{name}' k={k} w={w} filter={bf_o is not None} {way}")
                same(sub, exp, f"N-substituted '{name}' k={k} w={w} filter={bf_o is not None} {way}")
                if name in ("all records",):
                    assert got[0].size == 0
            # the same handle unmasked: the cached tables are untouched by the masked calls
            key = ("", w, bf_o is not None)
            if key not in case["exp"]:
                case["exp"][key] = oracle_flat(O.minimize(case["og"], k, w, bf_o))
            assert case["exp"][key][0].size > 50
            same(sketch(c, dg, k, w, bf_d).to_numpy(), case["exp"][key], f"unmasked after the masked calls k={k} w={w} filter={bf_o is not None} {way}")
    finally:
        reset(c)
        dbf.free()
        dg.free()


@pytest.mark.parametrize("k,w", [(24, 10), (24, 100), (24, 300), (129, 50)])
def test_masks_equal_n_substitution(ctx, k, w):
    masks_equal_substitution(ctx, k, w, lambda c: None, "auto")


@pytest.mark.parametrize("way", ["pruned", "tiers"])
@pytest.mark.parametrize("k,w", [(24, 300), (24, 100)])
def test_masks_equal_n_substitution_pruned_and_tiers(ctx, k, w, way):
    if way == "pruned":                                           # (one threshold: candidates listed, no tiers; the tiers: at least two planned)
        masks_equal_substitution(ctx, k, w, lambda c: c.sketch_mode("pruned"), way, lambda c: c.sketch_stats()[0] > 0 and c.sketch_tiers()[2] == 0)
    else:
        masks_equal_substitution(ctx, k, w, lambda c: c.sketch_tiers("always"), way, lambda c: c.sketch_tiers()[2] >= 2)


@pytest.mark.parametrize("use_bf", [False, True])
def test_masks_in_a_batch_address_the_batch_record_ids(ctx, use_bf):
    "two of the sets through Genome.concat of two such families: record ids rebased, the list splits into the per-family oracle lists"
    from ntsynt_amd.device import BloomFilter, Genome, sketch
    k, w = 24, 100
    a = mask_case(k)
    rng = np.random.default_rng(77)
    names_b, seqs_b, n_runs_b = SC.mask_family(k, rng)
    sets_a = dict(a["sets"])
    sets_b = dict(SC.mask_sets([len(s) for s in seqs_b], k, rng, n_runs_b))
    parts = [(a["names"], a["seqs"]), (names_b, seqs_b)]
    dg = [to_device(ctx, n, s) for n, s in parts]
    obf = dbf = None
    if use_bf:
        obf = a["obf"]
        dbf = BloomFilter(ctx, obf.size, k)
        dbf.from_numpy(obf)
    batch = Genome.concat(ctx, dg)
    try:
        for name_a, name_b in (("overlapping chains", "2000 short masks"), ("nested", "beyond the record")):
            per_part = [sets_a[name_a], sets_b[name_b]]
            masks = [(r + int(batch.rec_base[p]), s, e) for p, ms in enumerate(per_part) for r, s, e in ms]
            order = np.random.default_rng(3).permutation(len(masks))
            got = batch.split_minimizers(*sketch(ctx, batch, k, w, dbf, [masks[i] for i in order]).to_numpy())
            assert len(got) == 2
            for p, (names, seqs) in enumerate(parts):
                exp = oracle_flat(O.minimize(to_oracle(names, SC.apply_masks(seqs, per_part[p])), k, w, obf))
                assert exp[0].size > 50
                print(f"way=batch k={k} w={w} masks='{(name_a, name_b)[p]}' filter={use_bf} minimizers={got[p][0].size} uncovered_ranges={ctx.sketch_stats()[1]}")
                same(got[p], exp, f"batch part {p} masks '{(name_a, name_b)[p]}'")
                same(sketch(ctx, dg[p], k, w, dbf, per_part[p]).to_numpy(), exp, f"part {p} alone")
    finally:
        reset(ctx)
        batch.free()
        for d in dg:
            d.free()
        if dbf is not None:
            dbf.free()

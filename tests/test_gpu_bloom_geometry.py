"""The partitioned Bloom build (ntsynt_amd/csrc/nts_bloom_bin.inc: k_bin1, k_bin2, k_bin3, k_bin_late and the host plan) where it is
delicate, against the oracle, exactly: filter sizes whose final buckets do not divide evenly (buckets behind the filter's end, a
partial last bucket behind packed words, the scalar tails of k_bin3, the size whose plan used to ask for 513 level-1 buckets, a filter
of more than 2^32 bits), and the persistent loop of k_bin1 with several turns per workgroup (NTS_BIN1_GRID on the experiments build)
over tiles whose run boundaries, pieces, side-buffer and capacity overflows are placed on purpose.

The inputs are constructed (tests/bloom_cases.py; tests/test_bloom_cases_host.py checks on the CPU that they hold what is relied on
here).  Every expectation is O.bf_build, compared with np.array_equal.  Every test runs under a time limit of its own (a hung call ends
the process, with a traceback).  Needs an MI355X."""
import faulthandler
import subprocess
import sys

import numpy as np
import pytest

from oracle import nts_oracle as O
from tests import bloom_cases as BC
from tests.helpers import to_device, to_oracle

pytestmark = pytest.mark.gpu
STEP_SECONDS = 300
SWITCHES = ("NTS_BIN1_GRID", "NTS_BIN_STORE", "NTS_BIN_LATE_CAP", "NTS_BIN_IDX32")


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def ctx():
    from ntsynt_amd.device import Context
    cu_count()                                                    # (asked before the library's runtime comes up in this process: see there)
    c = Context(0)
    yield c
    c.close()


_cus = []


def cu_count():
    "torch.cuda.get_device_properties(0).multi_processor_count, asked once"
    if not _cus:
        import torch
        ask = "torch.cuda.get_device_properties(0).multi_processor_count"
        try:
            _cus.append(int(torch.cuda.get_device_properties(0).multi_processor_count))
        except RuntimeError:
            # torch brings a HIP runtime of its own, which may find no device in a process where the library's runtime came up first (a
            # run of other modules before this one): the same question in a fresh process
            out = subprocess.run([sys.executable, "-c", f"import torch; print({ask})"], capture_output=True, text=True, timeout=120, check=True)
            _cus.append(int(out.stdout.split()[-1]))
    return _cus[0]


def named(seqs):
    return [f"r{i}" for i in range(len(seqs))], seqs


def same(bf, want, what):
    got = bf.to_numpy()
    wide = np.uint64 if want.size % 8 == 0 else np.uint8          # (the same comparison, eight bytes at a time where the size allows)
    if got.size != want.size or not np.array_equal(got.view(wide), want.view(wide)):
        at = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {at.size} bytes of {want.size} differ from the oracle, first at byte {int(at[0])} "
                             f"(final bucket {int(at[0]) >> 13}): got {int(got[at[0]]):#04x}, expected {int(want[at[0]]):#04x}")


# ---- 1. bucket geometry, on the product build --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", list(BC.GEOMETRY))
def test_geometry_against_the_oracle(ctx, nbytes):
    """every finish of the build at this filter size: store-only into an empty filter, read-and-OR of a second genome, the AND of a
    2 % relative into the result (the oracle's cascade), the AND into an all-ones and into an empty filter"""
    from ntsynt_amd.device import BloomFilter
    (records, k, _, claims), (second, relative) = BC.geometry_case(nbytes)
    genomes = [named(s) for s in (records, second, relative)]
    og = [to_oracle(*g) for g in genomes]
    dg = [to_device(ctx, *g) for g in genomes]
    ctx.bf_build_mode("binned")
    bf = None
    try:
        bf = BloomFilter(ctx, nbytes, k)
        bf.insert(dg[0])                                          # the store-only finish
        want = O.bf_build(og[0], k, nbytes)
        pop = O.bf_popcount(want)
        print(f"nbytes={nbytes} ({claims['shape']}) kmers={dg[0].valid_kmers(k)} set bits={pop} bypassed={ctx.path_stats()['bf_direct_indices']}")
        assert bf.popcount() == pop
        same(bf, want, f"{nbytes} bytes, insert into an empty filter")
        bf.insert(dg[1])                                          # reads and ORs
        want |= O.bf_build(og[1], k, nbytes)
        same(bf, want, f"{nbytes} bytes, insert into a filter with content")
        bf.insert_and(dg[2])
        want = O.bf_build(og[2], k, nbytes, prev=want)
        assert 0 < O.bf_popcount(want) < pop
        same(bf, want, f"{nbytes} bytes, insert_and of a relative")
        assert bf.popcount() == O.bf_popcount(want)
        bf.free()
        bf = BloomFilter(ctx, nbytes, k, ones=True)
        bf.insert_and(dg[2])
        del want
        same(bf, O.bf_build(og[2], k, nbytes), f"{nbytes} bytes, insert_and into an all-ones filter")
        bf.free()
        bf = BloomFilter(ctx, nbytes, k)
        bf.insert_and(dg[2])
        assert bf.popcount() == 0                                 # (the build's own count; the bits themselves:)
        same(bf, np.zeros(nbytes, dtype=np.uint8), f"{nbytes} bytes, insert_and into an empty filter")
    finally:
        ctx.bf_build_mode("auto")
        if bf is not None:
            bf.free()
        for d in dg:
            d.free()


# ---- 2. the turns of k_bin1's workgroups, on the experiments build ----------------------------------------------------------------------
SEAM_NAMES = ("seams", "carried", "tiles1", "tiles2", "tiles3", "tiles4", "tiles5")
_cases = {}


def seam_case(name, k):
    "records, claims and per filter size (oracle filter, running filter with holes, their oracle cascade): built once, left unchanged"
    if (name, k) not in _cases:
        if len(_cases) > 2:
            _cases.clear()
        records, k, filters, claims = BC.repeat_case() if name == "repeat" else BC.seam_cases(k)[name]
        og = to_oracle(*named(records))
        per = {}
        for nbytes in filters:
            want = O.bf_build(og, k, nbytes)
            prev = want.copy()
            prev[::3] = 0                                          # a running filter that holds two thirds of the genome's bits
            prev[1::64] = 0xFF                                     # ... and bits the genome does not set
            per[nbytes] = (want, prev, O.bf_build(og, k, nbytes, prev=prev))
            assert 0 < O.bf_popcount(per[nbytes][2]) < O.bf_popcount(want) or O.bf_popcount(want) < 3
        _cases[(name, k)] = (records, claims, per)
    return _cases[(name, k)]


SEAM_CELLS = [(n, k, nbytes, grid) for n, ks in [(n, BC.SEAM_KS) for n in SEAM_NAMES] + [("repeat", (24,))]
              for k in ks for nbytes in BC.SEAM_FILTERS for grid in (1, 3, 4)]


@pytest.mark.parametrize("name,k,nbytes,grid", SEAM_CELLS)
def test_seams_and_turns_against_the_oracle(ctx_x, monkeypatch, name, k, nbytes, grid):
    """a grid of 1, 3 or 4 workgroups (3: the turns the case is built for), a one-level or a two-level filter: the store-only finish,
    read-and-OR (NTS_BIN_STORE=0), insert_and, and at grid 3 the first and the last with the parking list cut to three entries
    (NTS_BIN_LATE_CAP=3).  After every build the library says how many workgroups k_bin1 had: the switch took effect."""
    from ntsynt_amd.device import BloomFilter, bf_bin_plan
    c = ctx_x
    records, claims, per = seam_case(name, k)
    want, prev, want_and = per[nbytes]
    pop = O.bf_popcount(want)
    dg = to_device(c, *named(records))
    n_valid = dg.valid_kmers(k)
    plan = bf_bin_plan(n_valid, nbytes, k)
    shape = {"bin1_workgroups": min(grid, plan["tiles"]), "B1": plan["B1"], "log2_b2": plan["log2_b2"]}
    c.bf_build_mode("binned")
    bf = BloomFilter(c, nbytes, k)
    try:
        for mode in ("store", "read+or", "and") + (("store, list of 3", "and, list of 3") if grid == 3 else ()):
            for s in SWITCHES:
                monkeypatch.delenv(s, raising=False)
            monkeypatch.setenv("NTS_BIN1_GRID", str(grid))
            if mode == "read+or":
                monkeypatch.setenv("NTS_BIN_STORE", "0")
            if mode.endswith("list of 3"):
                monkeypatch.setenv("NTS_BIN_LATE_CAP", "3")
            what = f"{name} k={k} {nbytes} bytes grid={grid} {mode}"
            if mode.startswith("and"):
                bf.from_numpy(prev)
                bf.insert_and(dg)
                st = c.path_stats()
                same(bf, want_and, what)
            else:
                bf.clear()                                        # (a cleared filter counts as empty: the store-only finish)
                bf.insert(dg)
                st = c.path_stats()
                same(bf, want, what)
                assert bf.popcount() == pop, what
            assert c.bf_bin_last() == shape, what
            if claims.get("bypass"):                              # (in the AND build an index counts when the running filter holds its bit: two in three)
                assert st["bf_direct_indices"] > 0, what
            if mode.endswith("list of 3") and claims.get("bypass"):
                assert st["bf_list_fallback"] == 1, what
            if mode in ("store", "and"):
                print(f"{what}: kmers={n_valid} set bits={pop} bypassed={st['bf_direct_indices']} fallback={st['bf_list_fallback']}")
    finally:
        c.bf_build_mode("auto")
        bf.free()
        dg.free()


def test_the_grid_switch_does_nothing_on_the_product_build(ctx, monkeypatch):
    "NTS_BIN1_GRID=1 in the environment of the product build: k_bin1 still runs one workgroup per tile (thirteen tiles, far fewer than 2 per CU)"
    from ntsynt_amd.device import BloomFilter
    records, claims, per = seam_case("seams", 24)
    nbytes = BC.SEAM_FILTERS[0]
    dg = to_device(ctx, *named(records))
    ctx.bf_build_mode("binned")
    bf = BloomFilter(ctx, nbytes, 24)
    try:
        monkeypatch.setenv("NTS_BIN1_GRID", "1")
        bf.insert(dg)
        assert ctx.bf_bin_last()["bin1_workgroups"] == 13
        same(bf, per[nbytes][0], "the product build with NTS_BIN1_GRID set")
    finally:
        ctx.bf_build_mode("auto")
        bf.free()
        dg.free()


# ---- 3. no switches: the product build's own grid ----------------------------------------------------------------------------------------
def test_two_turns_of_the_product_grid_against_the_oracle(ctx):
    """2 * (2 * CUs) + 3 tiles: every workgroup of k_bin1's own grid takes a second tile, three a third, N runs in all three turns of two
    workgroups; level-1 buckets of several tiles, so that k_bin2 runs its unpredicated whole tiles and a partial last one"""
    from ntsynt_amd.device import BloomFilter
    cus = cu_count()
    records, k, nbytes, claims = BC.product_case(cus)
    rng = np.random.default_rng(9)
    a = np.frombuffer(records[0], dtype=np.uint8).copy()
    hit = (rng.random(a.size) < 0.02) & (a != ord("N"))
    a[hit] = BC.ACGT[rng.integers(0, 4, size=int(hit.sum()))]
    genomes = [named(records), named([BC.bases(rng, 70000), BC.bases(rng, 150000)]), named([a.tobytes()])]
    og = [to_oracle(*g) for g in genomes]
    dg = [to_device(ctx, *g) for g in genomes]
    ctx.bf_build_mode("binned")
    bf = BloomFilter(ctx, nbytes, k)
    try:
        bf.insert(dg[0])
        assert ctx.bf_bin_last() == {"bin1_workgroups": claims["grid"], "B1": 257, "log2_b2": 1}
        want = O.bf_build(og[0], k, nbytes)
        print(f"CUs={cus} tiles={claims['n_tiles']} kmers={dg[0].valid_kmers(k)} set bits={O.bf_popcount(want)} bypassed={ctx.path_stats()['bf_direct_indices']}")
        assert bf.popcount() == O.bf_popcount(want)
        same(bf, want, "insert into an empty filter")
        bf.insert(dg[1])
        want |= O.bf_build(og[1], k, nbytes)
        same(bf, want, "insert into a filter with content")
        bf.insert_and(dg[2])
        want = O.bf_build(og[2], k, nbytes, prev=want)
        same(bf, want, "insert_and of a relative")
        assert bf.popcount() == O.bf_popcount(want) > 0
    finally:
        ctx.bf_build_mode("auto")
        bf.free()
        for d in dg:
            d.free()

"""The partitioned Bloom build (ntsynt_amd/csrc/nts_bloom_bin.inc) on the three paths that tests/test_gpu_bloom_geometry.py does not reach,
each at the smallest shape that takes it, bit for bit against the oracle:

A. the second round of k_bin3's load loop: a final bucket of more than 16384 unpacked residues (filters of one and two final buckets)
   or more than 8192 packed words (32 MiB + 8 with 13 M k-mers), and a bucket clamped to cap1 > 16384; all five finishes of the
   geometry module against O.bf_build;
B. log2_b2 = 6 .. 9: filters of 2^30 + 8 to 2^34 bytes, where k_bin2 clears and scans up to 512 level-2 counters, and two sizes whose
   last level-1 bucket is partly real and is hit.  O.bf_build of 16 GiB is out of the question: the reference is the oracle's index
   set (bloom_cases.sparse_reference; tests/test_bloom_cases_host.py pins it to O.bf_build), the filter lives in a torch tensor and
   is compared on the device -- every non-zero byte of the reference has its value, nothing else is non-zero, and the popcount is
   the number of distinct indices.  Finishes: store-only, read-and-OR, insert_and of the relative, insert_and into an empty filter;
   the AND into an all-ones filter is left out at these sizes (16 GiB of ones need the whole reference dense);
C. idx32 == 0, the 64-bit place of a residue in the level-1 array (B1 * cap1 >= 2^32 in earnest), forced on the experiments build with
   NTS_BIN_IDX32=0: the seam cells and the case without switches of the geometry module again, against the same oracle filters.

The inputs are constructed (tests/bloom_cases.py; checked on the CPU by tests/test_bloom_cases_host.py).  Every test runs under a time
limit of its own.  Needs an MI355X."""
import faulthandler
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import nts_oracle as O
from tests import bloom_cases as BC
from tests import test_gpu_bloom_geometry as G
from tests.helpers import to_device, to_oracle

pytestmark = pytest.mark.gpu
CHILD = "NTS_BLOOM_LARGE_CHILD"                                   # set in the fresh process that child_outcomes() starts
CHILD_SECONDS = 240                                               # that whole process
STEP_SECONDS = 60 if os.environ.get(CHILD) else 300               # (a test that hangs there ends it, with its traceback, before the parent does)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def ctx():
    from ntsynt_amd.device import Context
    G.cu_count()                                                  # (torch's runtime before the library's: see there)
    c = Context(0)
    yield c
    c.close()


# ---- A. the second round of k_bin3's load loop -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BC.SECOND_TRIP))
def test_second_round_of_k_bin3_against_the_oracle(ctx, name):
    """the five finishes of the geometry module -- store-only, read-and-OR of a second genome, the AND of a 2 % relative, the AND into
    an all-ones and into an empty filter -- with final buckets that take a second trip through k_bin3's load loop"""
    from ntsynt_amd.device import BloomFilter, bf_bin_plan
    (records, k, nbytes, claims), (second, relative) = BC.second_trip_case(name)
    genomes = [G.named(s) for s in (records, second, relative)]
    og = [to_oracle(*g) for g in genomes]
    dg = [to_device(ctx, *g) for g in genomes]
    plan = bf_bin_plan(dg[0].valid_kmers(k), nbytes, k)
    ctx.bf_build_mode("binned")
    bf = None

    def binned(what, g, anded=False):
        """the finish just made went through the partitioned build -- k_bin1 had workgroups (the library resets the figure before it
        plans: a build that did not apply leaves 0), with this geometry -- and, an AND level, neither the literal way over a sparse
        filter nor a second time with a filter of the genome's own; its indices past the buckets"""
        last, st = ctx.bf_bin_last(idx32=True), ctx.path_stats()
        tiles = bf_bin_plan(dg[g].valid_kmers(k), nbytes, k)["tiles"]
        assert last == {"bin1_workgroups": min(tiles, 2 * G.cu_count()), "B1": plan["B1"], "log2_b2": plan["log2_b2"], "idx32": 1}, what
        assert st["bf_list_fallback"] == 0, what
        if anded:
            assert ctx.bf_level_stats()["sparse_level"] == 0, what
        else:                                                     # (in the AND build an index counts only when the running filter holds its bit)
            assert (st["bf_direct_indices"] > 0) == (claims["overflow"] and g != 1), f"{what}: {st['bf_direct_indices']} indices bypassed the buckets"
        return st["bf_direct_indices"]
    try:
        bf = BloomFilter(ctx, nbytes, k)
        bf.insert(dg[0])                                          # the store-only finish
        n_direct = binned(f"{name}, insert into an empty filter", 0)
        want = O.bf_build(og[0], k, nbytes)
        pop = O.bf_popcount(want)
        print(f"{name}: nbytes={nbytes} ({claims['shape']}) kmers={dg[0].valid_kmers(k)} set bits={pop} bypassed={n_direct}")
        assert bf.popcount() == pop
        G.same(bf, want, f"{name}, insert into an empty filter")
        bf.insert(dg[1])                                          # reads and ORs
        binned(f"{name}, insert into a filter with content", 1)
        want |= O.bf_build(og[1], k, nbytes)
        G.same(bf, want, f"{name}, insert into a filter with content")
        assert bf.popcount() == O.bf_popcount(want)
        bf.insert_and(dg[2])
        binned(f"{name}, insert_and of a relative", 2, anded=True)
        want = O.bf_build(og[2], k, nbytes, prev=want)
        assert 0 < O.bf_popcount(want) < pop
        G.same(bf, want, f"{name}, insert_and of a relative")
        assert bf.popcount() == O.bf_popcount(want)
        bf.free()
        bf = BloomFilter(ctx, nbytes, k, ones=True)
        bf.insert_and(dg[2])
        binned(f"{name}, insert_and into an all-ones filter", 2, anded=True)
        want = O.bf_build(og[2], k, nbytes)
        G.same(bf, want, f"{name}, insert_and into an all-ones filter")
        assert bf.popcount() == O.bf_popcount(want)
        bf.free()
        bf = BloomFilter(ctx, nbytes, k)
        bf.insert_and(dg[2])
        binned(f"{name}, insert_and into an empty filter", 2, anded=True)
        assert bf.popcount() == 0
        G.same(bf, np.zeros(nbytes, dtype=np.uint8), f"{name}, insert_and into an empty filter")
    finally:
        ctx.bf_build_mode("auto")
        if bf is not None:
            bf.free()
        for d in dg:
            d.free()


# ---- B. log2_b2 = 6 .. 9 -----------------------------------------------------------------------------------------------------------------
COUNT_PIECE = 1 << 30                                             # bytes counted at once: what torch needs beside the filter stays small


def same_sparse(tensor, bf, idx, nbytes, what):
    "the filter in `tensor` holds exactly the bits idx (sorted, distinct): every byte of the reference, no other byte, the popcount"
    import torch
    off, val = BC.sparse_bytes(idx)
    d_off = torch.from_numpy(off).to(tensor.device)
    got = tensor[d_off]
    bad = torch.nonzero(got != torch.from_numpy(val).to(tensor.device))
    if bad.numel():
        at = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of the reference's {off.size} bytes differ, first at byte {int(off[at])} (final bucket "
                             f"{int(off[at]) >> (BC.FINAL_SHIFT - 3)}): got {int(got[at]):#04x}, expected {int(val[at]):#04x}")
    starts = np.arange(0, tensor.numel(), COUNT_PIECE)
    nonzero = np.array([int(torch.count_nonzero(tensor[a:a + COUNT_PIECE])) for a in starts])
    if int(nonzero.sum()) != off.size:                            # (every byte of the reference is there: some other byte is set)
        expect = np.diff(np.searchsorted(off, np.append(starts, tensor.numel())))
        a = int(starts[np.flatnonzero(nonzero != expect)[0]])
        extra = np.setdiff1d(torch.nonzero(tensor[a:a + COUNT_PIECE]).flatten().cpu().numpy() + a, off)
        raise AssertionError(f"{what}: {int(nonzero.sum()) - off.size} bytes are set that the reference leaves zero, first at byte {int(extra[0])} "
                             f"(final bucket {int(extra[0]) >> (BC.FINAL_SHIFT - 3)}): got {int(tensor[int(extra[0])]):#04x}")
    assert tensor.numel() - nbytes < 16
    assert bf.popcount() == idx.size, what


_torch_here = []
_child = {}


def torch_here():
    """Whether torch finds the GPU in this process.  It brings a HIP runtime of its own, which finds no device where the library's
    runtime came up first (G.cu_count()): alone this module starts torch first (the `ctx` fixture); behind other GPU modules it cannot."""
    if not _torch_here:
        import torch
        try:
            torch.zeros(1, dtype=torch.uint8, device="cuda:0")
            _torch_here.append(True)
        except RuntimeError:
            _torch_here.append(False)
    return _torch_here[0]


def child_outcomes():
    """The tests of group B run once in a fresh process, where torch's runtime comes first: (nbytes -> outcome, the process's output).
    Started by the first of them that finds torch without a device; the others read what it left.  The process stops at its first
    failure (-x): nothing more is started on the GPU behind a size that went wrong, and the sizes behind it count as not passed.
    It is started ONCE whatever becomes of it: a process that ran out of time or could not be started leaves no outcome, and every
    size then fails on what is recorded here without starting anything."""
    if not _child:
        _child.update(outcomes={}, text="the fresh process was not started")          # (terminal from here on)
        if os.environ.get(CHILD):
            _child["text"] = "torch finds no GPU in a fresh process"
            return _child["outcomes"], _child["text"]
        try:
            out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-k", "test_large_geometry", "-x", "-q", "-rA",
                                  "-p", "no:cacheprovider"], cwd=ROOT, env=dict(os.environ, **{CHILD: "1"}), capture_output=True, text=True,
                                 timeout=CHILD_SECONDS)
        except subprocess.TimeoutExpired as e:
            def tail(b):
                return (b.decode(errors="replace") if isinstance(b, bytes) else b or "")[-6000:]
            _child["text"] = f"the fresh process did not end within {CHILD_SECONDS} s\n{tail(e.stdout)}\n{tail(e.stderr)}"
        except Exception as e:                                    # (whatever the launch raises: recorded, not tried again)
            _child["text"] = f"the fresh process could not be run: {type(e).__name__}: {e}"
        else:
            found = re.findall(r"^(PASSED|FAILED|ERROR) \S*::test_large_geometry_against_the_oracle_index_set\[(\d+)\]", out.stdout, flags=re.M)
            _child.update(outcomes={int(n): what for what, n in found}, text=f"exit status {out.returncode}\n{out.stdout[-6000:]}\n{out.stderr[-2000:]}")
    return _child["outcomes"], _child["text"]


@pytest.mark.parametrize("nbytes", list(BC.LARGE))
def test_large_geometry_against_the_oracle_index_set(ctx, nbytes):
    """store-only, read-and-OR of a second genome, the AND of a 2 % relative, and the AND into an empty filter, whose bytes all stay
    zero, at this filter size; one filter alive at a time.  (The AND into an all-ones filter stays with the sizes of the geometry
    module.)  In a process whose library runtime came up before torch's the same tests run once in a fresh process."""
    if torch_here():
        large_geometry(ctx, nbytes)
    else:
        outcomes, text = child_outcomes()
        assert outcomes.get(nbytes) == "PASSED", f"{nbytes} bytes, in a fresh process: {outcomes.get(nbytes, 'not run')}\n{text}"


def large_geometry(ctx, nbytes):
    import torch
    from ntsynt_amd.device import bf_bin_plan, wrap_bloom
    base = BC.large_base()
    k = BC.LARGE_K
    first, both, kept = BC.sparse_reference(base["h0"], nbytes)
    dg = [to_device(ctx, *G.named(g)) for g in base["genomes"]]
    plan = bf_bin_plan(dg[0].valid_kmers(k), nbytes, k)
    ctx.bf_build_mode("binned")
    tensor = bf = None

    def binned(g):
        "the finish just made went through the partitioned build, with this geometry (a build that did not apply leaves 0 workgroups)"
        tiles = bf_bin_plan(dg[g].valid_kmers(k), nbytes, k)["tiles"]
        assert ctx.bf_bin_last(idx32=True) == {"bin1_workgroups": min(tiles, 2 * G.cu_count()), "B1": plan["B1"], "log2_b2": plan["log2_b2"], "idx32": 1}
        assert ctx.path_stats()["bf_list_fallback"] == 0
    try:
        tensor = torch.zeros((nbytes + 15) // 16 * 16, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        bf = wrap_bloom(ctx, tensor, nbytes, k)
        bf.clear()                                                # (a cleared filter counts as empty: the store-only finish)
        bf.insert(dg[0])
        binned(0)
        print(f"nbytes={nbytes} ({BC.LARGE[nbytes]}) kmers={dg[0].valid_kmers(k)} set bits={first.size} bypassed={ctx.path_stats()['bf_direct_indices']}")
        same_sparse(tensor, bf, first, nbytes, f"{nbytes} bytes, insert into an empty filter")
        bf.insert(dg[1])                                          # reads and ORs
        binned(1)
        same_sparse(tensor, bf, both, nbytes, f"{nbytes} bytes, insert into a filter with content")
        bf.insert_and(dg[2])
        binned(2)
        assert 0 < kept.size < first.size
        same_sparse(tensor, bf, kept, nbytes, f"{nbytes} bytes, insert_and of a relative")
        bf.clear()
        bf.insert_and(dg[2])
        binned(2)
        for a in range(0, tensor.numel(), COUNT_PIECE):
            assert int(torch.count_nonzero(tensor[a:a + COUNT_PIECE])) == 0, f"{nbytes} bytes, insert_and into an empty filter: bytes set from {a} on"
        assert bf.popcount() == 0
    finally:
        ctx.bf_build_mode("auto")
        if bf is not None:
            bf.free()
        del tensor
        torch.cuda.empty_cache()
        for d in dg:
            d.free()


# ---- C. idx32 == 0 at small size, on the experiments build -------------------------------------------------------------------------------
def direct_slack(plan, direct):
    """By how much the indices past the buckets of two builds of the same genome may differ.  Past the buckets go the lanes that the side
    buffer does not hold and whatever a level-1 bucket holds beyond cap1: the same number in any order of the workgroups.  Behind k_bin2
    the number depends on how the residues fall into words: by at most two residues for every partly filled word, one per tile of
    k_bin2 and final bucket.  A build in which nothing went past the buckets is far from every capacity: none in the other either.
    So the comparison is exact in every one-level cell and wherever nothing bypasses; in a two-level cell with bypasses (the seams
    and the repeat case at 32 MiB + 8: 1028 indices of slack) it is loose on purpose and sees only a build that fell to the direct
    path wholesale -- which the one-level cell of the same case sees exactly."""
    return 2 * plan["tiles2"] * plan["n_final"] if plan["log2_b2"] and direct else 0


@pytest.mark.parametrize("name,k,nbytes,grid", G.SEAM_CELLS)
def test_seams_and_turns_with_the_64_bit_place(ctx_x, monkeypatch, name, k, nbytes, grid):
    """the cells of the geometry module's section 2 with NTS_BIN_IDX32=0: store-only, read-and-OR, insert_and (and at grid 3 the first and
    the last with a parking list of three entries), each first as the plan has it -- the library reports idx32 = 1 -- and then forced --
    idx32 = 0, the same filter, and the same number of indices past the buckets: a place that came out wrong and fell to the direct path
    would still give the right bits."""
    from ntsynt_amd.device import BloomFilter, bf_bin_plan
    c = ctx_x
    records, claims, per = G.seam_case(name, k)
    want, prev, want_and = per[nbytes]
    pop = O.bf_popcount(want)
    dg = to_device(c, *G.named(records))
    plan = bf_bin_plan(dg.valid_kmers(k), nbytes, k)
    assert plan["idx32"] == 1
    shape = {"bin1_workgroups": min(grid, plan["tiles"]), "B1": plan["B1"], "log2_b2": plan["log2_b2"]}
    c.bf_build_mode("binned")
    bf = BloomFilter(c, nbytes, k)
    try:
        for mode in ("store", "read+or", "and") + (("store, list of 3", "and, list of 3") if grid == 3 else ()):
            direct = {}
            for idx32 in (1, 0):
                for s in G.SWITCHES:
                    monkeypatch.delenv(s, raising=False)
                monkeypatch.setenv("NTS_BIN1_GRID", str(grid))
                if idx32 == 0:
                    monkeypatch.setenv("NTS_BIN_IDX32", "0")
                if mode == "read+or":
                    monkeypatch.setenv("NTS_BIN_STORE", "0")
                if mode.endswith("list of 3"):
                    monkeypatch.setenv("NTS_BIN_LATE_CAP", "3")
                what = f"{name} k={k} {nbytes} bytes grid={grid} {mode} idx32={idx32}"
                if mode.startswith("and"):
                    bf.from_numpy(prev)
                    bf.insert_and(dg)
                else:
                    bf.clear()
                    bf.insert(dg)
                st = c.path_stats()
                assert c.bf_bin_last(idx32=True) == dict(shape, idx32=idx32), what
                direct[idx32] = st["bf_direct_indices"]
                if idx32 == 0:                                    # (as the plan has it: the geometry module compares that build)
                    G.same(bf, want_and if mode.startswith("and") else want, what)
                    if not mode.startswith("and"):
                        assert bf.popcount() == pop, what
                    if claims.get("bypass"):
                        assert st["bf_direct_indices"] > 0, what
            if not mode.startswith("and"):                        # (in the AND build an index counts when it is the first to find its bit: no such figure)
                assert abs(direct[0] - direct[1]) <= direct_slack(plan, direct[1]), \
                    f"{name} k={k} {nbytes} bytes grid={grid} {mode}: {direct[0]} indices past the buckets, {direct[1]} with idx32 = 1"
    finally:
        c.bf_build_mode("auto")
        bf.free()
        dg.free()


def test_two_turns_of_the_product_grid_with_the_64_bit_place(ctx_x, monkeypatch):
    "the geometry module's case without switches -- k_bin1's own grid, two and three tiles per workgroup -- with NTS_BIN_IDX32=0 alone"
    from ntsynt_amd.device import BloomFilter, bf_bin_plan
    c = ctx_x
    cus = G.cu_count()
    records, k, nbytes, claims = BC.product_case(cus)
    rng = np.random.default_rng(9)
    a = np.frombuffer(records[0], dtype=np.uint8).copy()
    hit = (rng.random(a.size) < 0.02) & (a != ord("N"))
    a[hit] = BC.ACGT[rng.integers(0, 4, size=int(hit.sum()))]
    genomes = [G.named(records), G.named([BC.bases(rng, 70000), BC.bases(rng, 150000)]), G.named([a.tobytes()])]
    og = [to_oracle(*g) for g in genomes]
    dg = [to_device(c, *g) for g in genomes]
    for s in G.SWITCHES:
        monkeypatch.delenv(s, raising=False)
    c.bf_build_mode("binned")
    bf = BloomFilter(c, nbytes, k)
    shape = {"bin1_workgroups": claims["grid"], "B1": 257, "log2_b2": 1}
    try:
        bf.insert(dg[0])
        assert c.bf_bin_last(idx32=True) == dict(shape, idx32=1)
        direct = c.path_stats()["bf_direct_indices"]
        monkeypatch.setenv("NTS_BIN_IDX32", "0")
        bf.clear()
        bf.insert(dg[0])
        assert c.bf_bin_last(idx32=True) == dict(shape, idx32=0)
        assert abs(c.path_stats()["bf_direct_indices"] - direct) <= direct_slack(bf_bin_plan(dg[0].valid_kmers(k), nbytes, k), direct)
        want = O.bf_build(og[0], k, nbytes)
        assert bf.popcount() == O.bf_popcount(want)
        G.same(bf, want, "idx32 = 0, insert into an empty filter")
        bf.insert(dg[1])
        want |= O.bf_build(og[1], k, nbytes)
        G.same(bf, want, "idx32 = 0, insert into a filter with content")
        bf.insert_and(dg[2])
        assert c.bf_bin_last(idx32=True) == dict(shape, idx32=0)
        want = O.bf_build(og[2], k, nbytes, prev=want)
        G.same(bf, want, "idx32 = 0, insert_and of a relative")
        assert bf.popcount() == O.bf_popcount(want) > 0
    finally:
        c.bf_build_mode("auto")
        bf.free()
        for d in dg:
            d.free()

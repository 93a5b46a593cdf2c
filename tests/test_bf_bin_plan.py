"""nts_bf_bin_plan, the host plan of the partitioned Bloom build (include/ntsynt_hip.h; ntsynt_amd/csrc/nts_bloom_bin.inc: bf_bin_plan,
which bf_insert_binned calls): the bucket geometry for every filter size the build can meet, against the limits its kernels are
compiled with -- k_bin1 keeps two LDS tables of BIN_MAX_B1 = 512 level-1 buckets, k_bin2 three of 2^9 level-2 buckets and addresses
the level-2 buckets of a level-1 bucket with 30-bit word offsets, k_bin3 reads its residues sixteen bytes at a time.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

from ntsynt_amd import _lib
from ntsynt_amd.device import BF_BIN_PLAN_FIELDS, bf_bin_plan
from tests.test_gpu_bloom_geometry import SWITCHES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUCKET_BYTES = 65536                      # a final bucket: 2^19 filter bits
MAX_B1, MAX_LOG2_B2 = 512, 9
V_LIMIT = 0xFF000000
VS = (1, 8191, 8192, 8193, 1 << 22, 3 * 10**9, V_LIMIT - 1, V_LIMIT)
NF = len(BF_BIN_PLAN_FIELDS)


def plans(n_valid, nbytes, k=24, forced=True, and_mode=False):
    "the plan of every byte count in `nbytes`: (rc per call, dict of uint64 columns)"
    f = _lib.load().nts_bf_bin_plan
    nbytes = [int(b) for b in nbytes]
    buf = (ctypes.c_uint64 * (NF * len(nbytes)))()
    at = ctypes.addressof(buf)
    rc = [f(n_valid, b, k, int(forced), int(and_mode), at + 8 * NF * i) for i, b in enumerate(nbytes)]
    rows = np.frombuffer(buf, dtype=np.uint64).reshape(len(nbytes), NF)
    return np.array(rc), {name: rows[:, i].astype(np.int64) for i, name in enumerate(BF_BIN_PLAN_FIELDS)}


def check(n_valid, nbytes, k=24, forced=True, and_mode=False):
    nbytes = np.asarray(nbytes, dtype=np.int64)
    rc, p = plans(n_valid, nbytes, k, forced, and_mode)
    assert set(np.unique(rc)) <= {0, 1}
    F = (nbytes * 8 + (1 << 19) - 1) >> 19
    # ---- the tables of k_bin1 first: what every other number is derived from ----------------------------------------------------------
    bad = np.flatnonzero(p["B1"] > MAX_B1)
    assert bad.size == 0, f"B1 = {p['B1'][bad[0]]} at F = {F[bad[0]]} ({nbytes[bad[0]]} bytes, V = {n_valid}): k_bin1's LDS tables hold {MAX_B1} buckets; {bad.size} such sizes"
    # ---- the refusals -------------------------------------------------------------------------------------------------------------
    named = np.zeros(nbytes.size, dtype=bool)
    if n_valid == 0 or n_valid >= V_LIMIT or (and_mode and k > 128):
        named[:] = True
    named |= nbytes * 8 > (1 << 37)                              # filter beyond 2^37 bits
    if not forced:
        named |= (F < 64) | (n_valid < (1 << 22))                # too small to pay for three passes
    assert (rc[named] == 1).all(), f"V={n_valid}: applies where the build is refused, first at {nbytes[named & (rc == 0)][:3]} bytes"
    # (beside the named ones: capacities that do not fit 31 bits -- billions of k-mers into a handful of buckets)
    fits = n_valid * 1.2 / np.minimum(F, MAX_B1).clip(1) + 8192 < (1 << 31)
    must = ~named & fits
    assert (rc[must] == 0).all(), f"V={n_valid}: refused without a reason, first at {nbytes[must & (rc == 1)][:3]} bytes"
    on = rc == 0
    for name in BF_BIN_PLAN_FIELDS:                              # a refused plan holds zeros
        assert not np.any(p[name][~on] != 0), name
    if not on.any():
        return 0
    F, q = F[on], {name: col[on] for name, col in p.items()}
    # ---- the geometry -------------------------------------------------------------------------------------------------------------
    assert (q["F"] == F).all()
    assert (q["log2_b2"] <= MAX_LOG2_B2).all() and (q["B2"] == 1 << q["log2_b2"]).all()
    assert (q["n_final"] == q["B1"] * q["B2"]).all()
    assert (q["n_final"] >= F).all() and (q["n_final"] - F < q["B2"]).all()
    assert (q["B1"] == (F + q["B2"] - 1) // q["B2"]).all()
    # (the smallest B2 that does: no second level where one is enough)
    assert ((q["log2_b2"] == 0) | ((F + q["B2"] // 2 - 1) // (q["B2"] // 2).clip(1) > MAX_B1)).all()
    cap1, cap2 = q["cap1"], q["cap2"]                            # (below 2^31 each, or the plan refuses: the products fit 64 bits)
    assert (cap1 % 4 == 0).all() and (cap1 * q["B1"] >= n_valid).all()                         # (mean and more: uniform hashes fit)
    assert (cap2 % 2 == 0).all() and ((cap2 << q["log2_b2"]) < (1 << 30)).all() and ((cap2 == 0) == (q["log2_b2"] == 0)).all()
    assert (q["idx32"] == (q["B1"] * cap1 < (1 << 32))).all()
    assert (q["tiles"] == (n_valid + 8191) // 8192).all() and (q["tiles2"] == (cap1 + 8191) // 8192).all()
    return int(on.sum())


@pytest.mark.parametrize("n_valid", VS)
def test_every_number_of_final_buckets(n_valid):
    "every F from 1 to 2^18 + 1024 (2^18 final buckets are 2^37 bits), as the last byte count that gives it"
    F = np.arange(1, (1 << 18) + 1024 + 1, dtype=np.int64)
    n = check(n_valid, F * BUCKET_BYTES)
    assert (n > 0) == (n_valid < V_LIMIT)


def edge_sizes():
    out = []
    for j in range(MAX_LOG2_B2 + 1):
        top = MAX_B1 * (1 << j) * BUCKET_BYTES                   # the largest filter with B2 = 2^j
        for d in (-BUCKET_BYTES, -13, -8, -1, 0, 1, 8, 13, BUCKET_BYTES):
            out.append(top + d)
    return out


@pytest.mark.parametrize("and_mode", [False, True])
@pytest.mark.parametrize("forced", [True, False])
@pytest.mark.parametrize("n_valid", VS)
def test_around_every_change_of_level(n_valid, forced, and_mode):
    "byte counts around each 512 * 2^j buckets, where log2_b2 steps: 8 bytes and one bucket to either side"
    for k in (24, 128, 129):
        check(n_valid, edge_sizes(), k, forced, and_mode)


def test_the_smallest_size_that_rounded_past_the_tables():
    "F = 1025 (64 MiB + 8): 1025 >> 1 is 512, ceil(1025 / 2) is 513 -- two level-2 buckets are not enough, four are"
    p = bf_bin_plan(300000, (64 << 20) + 8)
    assert {n: p[n] for n in ("F", "log2_b2", "B2", "B1", "n_final", "tiles", "tiles2", "idx32")} == \
        dict(F=1025, log2_b2=2, B2=4, B1=257, n_final=1028, tiles=37, tiles2=1, idx32=1)
    p = bf_bin_plan(300000, (1 << 29) + 8)
    assert (p["F"], p["B2"], p["B1"], p["n_final"]) == (8193, 32, 257, 8224)
    assert bf_bin_plan(300000, (32 << 20) + 8)["B1"] == 257 and bf_bin_plan(300000, 64 << 20)["B1"] == 512


def test_refusals_and_bad_arguments():
    assert bf_bin_plan(0, 1 << 20) is None                       # nothing to build
    assert bf_bin_plan(1000, 0) is None
    assert bf_bin_plan(V_LIMIT, 1 << 30) is None and bf_bin_plan(V_LIMIT - 1, 1 << 30) is not None
    assert bf_bin_plan(1 << 22, (1 << 34) + 1) is None and bf_bin_plan(1 << 22, 1 << 34) is not None        # 2^37 bits
    assert bf_bin_plan(1 << 22, 1 << 62) is None
    assert bf_bin_plan(1 << 22, 64 << 20, k=129, and_mode=True) is None and bf_bin_plan(1 << 22, 64 << 20, k=129) is not None
    assert bf_bin_plan((1 << 22) - 1, 64 << 20, forced=False) is None and bf_bin_plan(1 << 22, 64 << 20, forced=False) is not None
    assert bf_bin_plan(1 << 22, 63 * BUCKET_BYTES, forced=False) is None
    assert _lib.load().nts_bf_bin_plan(1000, 1 << 20, 24, 1, 0, None) == -22


def test_the_grid_switch_is_not_in_the_product_build():
    "NTS_BIN1_GRID (k_bin1's workgroups, for the tests) reaches the library through NTS_KNOB: the name is in the experiments build alone"
    def holds(lib):
        with open(os.path.join(ROOT, "ntsynt_amd", lib), "rb") as fh:
            return b"NTS_BIN1_GRID" in fh.read()
    assert holds("libntsynt_hip_exp.so") and not holds("libntsynt_hip.so")


@pytest.mark.parametrize("switch", SWITCHES)
def test_no_switch_of_the_bloom_tests_is_in_the_product_build(switch):
    "every switch the GPU tests of the partitioned build set (NTS_BIN_IDX32 among them: the 64-bit place on a small genome): in the experiments build alone"
    def holds(lib):
        with open(os.path.join(ROOT, "ntsynt_amd", lib), "rb") as fh:
            return switch.encode("ascii") in fh.read()
    assert "NTS_BIN_IDX32" in SWITCHES and holds("libntsynt_hip_exp.so") and not holds("libntsynt_hip.so")

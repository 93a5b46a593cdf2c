"""nts_cigar_build (csrc/nts_cigar.inc, Context.cigar_build; docs/design/04_22_block_alignments.md) against tests/cigar_brute.py, entry for
entry and record for record, on the smallest shapes at which the kernels can go wrong: one piece without an op; empty pieces between
others; no piece, and chains without pieces in front, in the middle and at the end; an op at p = 0 and an op that ends its piece; runs
of one kind inside a piece, across a piece border and NOT across a chain border; reversed pieces alone, in front of forward ones and
with an indel at their far end; one `=` run over 3 000 pieces and a chain of 70 000 atoms (runs and chains that straddle workgroups
and scan tiles); two pieces of 2^31 + 1 bases (one entry longer than 2^32; no genome is read); 2 000 random pieces in 300 chains with
the canonical scripts of tests/variants_brute.py on random short strings; every refusal, each naming the smallest offender and
returning nothing, a seg that is no piece's index and lengths that add up to 2^60 among them; the same bytes twice.  Every case's expectation is computed on the CPU before the GPU is called.  Every test runs
under a time limit of its own."""
import ctypes
import faulthandler

import numpy as np
import pytest

from tests import cigar_brute as CB
from tests import variants_brute as V

pytestmark = pytest.mark.gpu
STEP_SECONDS = 300
SUB, DEL, INS = CB.SUB, CB.DEL, CB.INS
REV = CB.REVERSED
FIELDS = ("first", "n_cig", "eq", "x", "ins", "del", "len_a", "len_b")


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def ctx():
    from ntsynt_amd.device import Context
    c = Context(0)
    c.profile(True)
    yield c
    c.close()


def arrays(pieces, scripts):
    "pieces: (chain, n, m, flags); scripts: per piece its (op, p, q) list.  Returns (PIECE array, OP array with seg = the piece, first)"
    from ntsynt_amd.device import OP_DTYPE, PIECE_DTYPE
    pc = np.array([tuple(p) for p in pieces], dtype=PIECE_DTYPE) if pieces else np.zeros(0, dtype=PIECE_DTYPE)
    ops = [(t, p, q, op, 0xFF, 0xFF, 0) for t, s in enumerate(scripts) for op, p, q in s]
    first = np.concatenate([[0], np.cumsum([len(s) for s in scripts])]).astype(np.uint64)
    return pc, (np.array(ops, dtype=OP_DTYPE) if ops else np.zeros(0, dtype=OP_DTYPE)), first


def check(ctx, pieces, scripts, n_chains, what, want_text=None):
    from ntsynt_amd.device import CHAIN_DTYPE
    pc, ops, first = arrays(pieces, scripts)
    entries, chains = CB.brute_cigar(pc.tolist(), ops.tolist(), first, n_chains)
    if want_text is not None:
        assert [CB.cigar_string(entries[c["first"]:c["first"] + c["n_cig"]]) for c in chains] == want_text, what
    got, recs = ctx.cigar_build(pc, ops, first, n_chains)
    again, recs_again = ctx.cigar_build(pc, ops, first, n_chains)
    assert got.dtype == np.uint64 and recs.dtype == CHAIN_DTYPE and recs.shape == (n_chains,)
    print(f"{what}: {len(pieces)} pieces, {ops.size} ops, {n_chains} chains, {len(entries)} entries (got {got.size})")
    assert got.tolist() == entries, (what, CB.cigar_string(got[:20]), CB.cigar_string(entries[:20]))
    assert [tuple(int(v) for v in r) for r in recs] == [tuple(c[f] for f in FIELDS) for c in chains], what
    assert got.tobytes() == again.tobytes() and recs.tobytes() == recs_again.tobytes(), what
    return got, recs


def test_one_piece_without_an_op_is_one_entry(ctx):
    got, recs = check(ctx, [(0, 17, 17, 0)], [[]], 1, "one piece", ["17="])
    assert got.tolist() == [17 << 4 | 7] and int(recs[0]["eq"]) == 17


def test_empty_pieces_between_others(ctx):
    check(ctx, [(0, 0, 0, 0), (0, 5, 5, 0), (0, 0, 0, 0), (0, 0, 0, REV), (0, 4, 4, 0), (0, 0, 0, 0)], [[]] * 6, 1, "empty pieces", ["9="])
    check(ctx, [(0, 0, 0, 0), (1, 0, 0, 0)], [[], []], 2, "only empty pieces", ["", ""])


def test_no_piece_and_chains_without_pieces(ctx):
    launches = ctx.timing("cigar_atoms")[1]
    got, recs = check(ctx, [], [], 3, "no piece", ["", "", ""])
    assert ctx.timing("cigar_atoms")[1] == launches and got.size == 0                      # (nothing was launched)
    check(ctx, [], [], 0, "no piece, no chain", [])
    _, recs = check(ctx, [(1, 3, 3, 0), (3, 2, 3, 0)], [[], [(INS, 2, 2)]], 6, "chains without pieces in front, in the middle, at the end",
                    ["", "3=", "", "2=1I", "", ""])
    assert [int(r["first"]) for r in recs] == [0, 0, 1, 1, 3, 3]


def test_ops_at_either_end_of_a_piece(ctx):
    check(ctx, [(0, 4, 4, 0)], [[(SUB, 0, 0)]], 1, "an op at p = 0", ["1X3="])
    check(ctx, [(0, 4, 4, 0)], [[(SUB, 3, 3)]], 1, "an op that ends the piece", ["3=1X"])
    check(ctx, [(0, 1, 0, 0)], [[(DEL, 0, 0)]], 1, "a piece that is one deletion", ["1D"])
    check(ctx, [(0, 0, 2, 0)], [[(INS, 0, 0), (INS, 0, 1)]], 1, "a piece that is one insertion", ["2I"])
    check(ctx, [(0, 4, 3, 0)], [[(DEL, 3, 3)]], 1, "a deletion at q = m", ["3=1D"])
    check(ctx, [(0, 3, 4, 0)], [[(INS, 3, 3)]], 1, "an insertion at p = n", ["3=1I"])


def test_runs_inside_a_piece(ctx):
    check(ctx, [(0, 8, 5, 0)], [[(DEL, 2, 2), (DEL, 3, 2), (DEL, 4, 2)]], 1, "DEL DEL DEL", ["2=3D3="])
    check(ctx, [(0, 6, 6, 0)], [[(SUB, 2, 2), (SUB, 3, 3)]], 1, "two SUBs", ["2=2X2="])
    check(ctx, [(0, 5, 5, 0)], [[(INS, 2, 2), (DEL, 2, 3)]], 1, "INS next to DEL", ["2=1I1D2="])
    check(ctx, [(0, 5, 5, 0)], [[(DEL, 2, 2), (INS, 3, 2)]], 1, "DEL next to INS", ["2=1D1I2="])


def test_runs_across_piece_borders_but_not_chain_borders(ctx):
    check(ctx, [(0, 3, 3, 0), (0, 3, 3, 0)], [[(SUB, 2, 2)], [(SUB, 0, 0)]], 1, "SUB | SUB in one chain", ["2=2X2="])
    check(ctx, [(0, 3, 3, 0), (1, 3, 3, 0)], [[(SUB, 2, 2)], [(SUB, 0, 0)]], 2, "SUB | SUB in two chains", ["2=1X", "1X2="])
    got, _ = check(ctx, [(0, 3, 3, 0), (1, 4, 4, 0)], [[], []], 2, "= | = in two chains", ["3=", "4="])
    assert got.size == 2
    check(ctx, [(0, 2, 1, 0), (0, 0, 0, 0), (0, 2, 1, 0)], [[(DEL, 1, 1)], [], [(DEL, 0, 0)]], 1, "DEL | empty | DEL", ["1=2D1="])


def test_reversed_pieces(ctx):
    check(ctx, [(0, 5, 6, REV)], [[(SUB, 1, 1), (INS, 4, 4)]], 1, "a reversed piece alone", ["1=1I2=1X1="])
    check(ctx, [(0, 5, 6, REV), (0, 3, 3, 0), (0, 2, 2, 0)], [[(SUB, 1, 1), (INS, 4, 4)], [], [(SUB, 1, 1)]], 1, "reversed in front of forward pieces",
          ["1=1I2=1X5=1X"])
    check(ctx, [(0, 6, 4, REV), (0, 3, 3, 0)], [[(SUB, 0, 0), (DEL, 4, 4), (DEL, 5, 4)], []], 1, "an indel at the far end", ["2D3=1X3="])
    check(ctx, [(0, 3, 3, REV), (0, 3, 3, 0)], [[(SUB, 0, 0)], [(SUB, 0, 0)]], 1, "reversed SUB meets forward SUB", ["2=2X2="])


def test_a_run_and_a_chain_across_workgroups_and_scan_tiles(ctx):
    got, recs = check(ctx, [(0, 7 + t % 5, 7 + t % 5, t % 2 * REV) for t in range(3000)], [[]] * 3000, 1, "one = run over 3 000 pieces")
    assert got.size == 1 and int(got[0]) >> 4 == sum(7 + t % 5 for t in range(3000))
    # pieces of 700 bases with a SUB at every 7th base (100 ops, 201 atoms each): 5 in chain 0, 350 in chain 1 (70 350 atoms), 5 in chain 2
    scripts = [[(SUB, p, p) for p in range(6 if t % 3 else 0, 700, 7)] for t in range(360)]
    pieces = [(0 if t < 5 else 1 if t < 355 else 2, 700, 700, REV if t % 4 == 1 else 0) for t in range(360)]
    assert sum(2 * len(s) + 1 for s, p in zip(scripts, pieces) if p[0] == 1) >= 70_000
    check(ctx, pieces, scripts, 3, "70 000 atoms")


def test_lengths_beyond_32_bits(ctx):
    big = 2 ** 31 + 1
    got, recs = check(ctx, [(0, big, big, 0), (0, big, big, 0)], [[], []], 1, "two pieces of 2^31 + 1 bases", [f"{2 ** 32 + 2}="])
    assert got.tolist() == [(2 ** 32 + 2) << 4 | 7] and int(recs[0]["len_a"]) == 2 ** 32 + 2


def random_case(seed, n_pieces=2000, n_chains=300):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    chain = np.sort(rng.integers(0, n_chains, n_pieces))
    pieces, scripts = [], []
    for t in range(n_pieces):
        a = letters[rng.integers(0, 4, int(rng.integers(0, 24)))]
        kind = int(rng.integers(0, 4))
        if kind == 0:
            b = a.copy()
        elif kind == 1:
            b = letters[rng.integers(0, 4, int(rng.integers(0, 24)))]
        else:                                                 # a few edits
            b = a.tolist()
            for _ in range(int(rng.integers(1, 4))):
                at = int(rng.integers(0, len(b) + 1))
                what = int(rng.integers(0, 3))
                if what == 0 and at < len(b):
                    b[at] = int(letters[rng.integers(0, 4)])
                elif what == 1 and at < len(b):
                    del b[at]
                else:
                    b.insert(at, int(letters[rng.integers(0, 4)]))
            b = np.array(b, dtype=np.uint8)
        scripts.append(V.script(a, b))
        pieces.append((int(chain[t]), a.size, b.size, REV if t % 3 == 0 else 0))
    return pieces, scripts


def test_random_pieces(ctx):
    pieces, scripts = random_case(7)
    assert sum(1 for p in pieces if p[3]) > 600 and sum(len(s) for s in scripts) > 3000
    check(ctx, pieces, scripts, 300, "2 000 random pieces in 300 chains")


def refused(ctx, pc, ops, first, n_chains, code, *words, n_pieces=None):
    "the call through the library itself: the return code, the message, nothing written.  n_pieces: a count other than the array's"
    from ntsynt_amd.device import CHAIN_DTYPE
    chains = np.full(max(min(int(n_chains), 8), 1), 0xAB, dtype=np.uint8).repeat(CHAIN_DTYPE.itemsize).view(CHAIN_DTYPE)
    before = chains.tobytes()
    p, m = ctypes.c_void_p(0x1234), ctypes.c_uint64(77)
    rc = ctx.lib.nts_cigar_build(ctx.h, pc.ctypes.data if pc.size else None, pc.size if n_pieces is None else int(n_pieces), int(n_chains), ops.ctypes.data if ops.size else None,
                                 first.ctypes.data, ctypes.byref(p), ctypes.byref(m), chains.ctypes.data)
    said = ctx.lib.nts_last_error(ctx.h).decode()
    print(rc, said)
    assert rc == code and all(w in said for w in words), (rc, said, words)
    assert chains.tobytes() == before
    assert (p.value, m.value) in ((0x1234, 77), (None, 0))    # (untouched before the launch; NULL and 0 behind it)
    return said


def test_refusals_before_any_launch(ctx):
    launches = ctx.timing("cigar_atoms")[1]
    ok = [(0, 3, 3, 0), (1, 3, 3, 0), (1, 3, 3, 0), (2, 3, 3, 0)]
    pc, ops, first = arrays(ok, [[], [(SUB, 0, 0)], [], []])
    for t, field, value, words in ((2, "chain", 0, ("piece 2", "chain order")), (3, "chain", 3, ("piece 3", "n_chains")), (1, "flags", 2, ("piece 1", "flag")),
                                   (0, "flags", 0x80000000, ("piece 0", "flag"))):
        bad = pc.copy()
        bad[field][t] = value
        bad["flags"][3] = 4 if t < 3 else bad["flags"][3]   # (a later offender as well: the smallest one is named)
        refused(ctx, bad, ops, first, 3, -22, *words)
    late = pc.copy()
    late["chain"] = [1, 0, 1, 0]                              # descending at piece 1 and again at piece 3
    refused(ctx, late, ops, first, 3, -22, "piece 1", "chain order")
    refused(ctx, pc, ops, np.array([0, 0, 1, 0, 1], dtype=np.uint64), 3, -22, "piece 2", "nondecreasing")
    refused(ctx, pc, ops, np.array([1, 1, 1, 1, 1], dtype=np.uint64), 3, -22, "piece 0", "start at 0")
    refused(ctx, pc, ops, first, 2 ** 32, -34, "2^32")
    refused(ctx, pc, ops, first, 3, -34, "2^32", n_pieces=2 ** 32)                                  # refused before any piece is read
    refused(ctx, pc[:1], ops[:0], np.array([0, 2 ** 31], dtype=np.uint64), 3, -34, "2^32")          # 2 n_ops + n_pieces = 2^32 + 1: no op is read
    assert ctx.timing("cigar_atoms")[1] == launches


def test_lengths_that_add_up_to_2_to_60_are_refused(ctx):
    """len << 4 must fit 64 bits.  Pieces hold at most 2^32 - 1 bases a side, so the sum reaches 2^60 only behind 2^27 pieces: the
    smallest such input, 2 GiB of pieces, none of which is sent to the GPU"""
    from ntsynt_amd.device import PIECE_DTYPE
    launches = ctx.timing("cigar_atoms")[1]
    n = 2 ** 27 + 1
    assert (n - 1) * 2 * (2 ** 32 - 1) < 2 ** 60 <= n * 2 * (2 ** 32 - 1)                           # the last piece crosses the limit
    words = np.empty((n, 4), dtype=np.uint32)
    words[:] = (0, 2 ** 32 - 1, 2 ** 32 - 1, 0)
    refused(ctx, words.reshape(-1).view(PIECE_DTYPE), np.zeros(0, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64), 1, -34, "2^60")
    assert ctx.timing("cigar_atoms")[1] == launches


@pytest.mark.parametrize("what, script", [
    ("p - i != q - j", [(SUB, 2, 3)]), ("an op behind its predecessor", [(SUB, 3, 3), (SUB, 3, 3)]), ("an op beyond n", [(SUB, 6, 6)]),
    ("a DEL at p = n", [(DEL, 6, 6)]), ("an INS at q = m", [(INS, 6, 6)]), ("op code 0", [(0, 1, 1)]), ("op code 4", [(4, 1, 1)]),
    ("the trailing run leaves the diagonal", [(DEL, 2, 2)]), ("a wrong seg", "seg"), ("a seg at n_pieces", "seg 5"), ("a seg of 2^32 - 1", "seg 4294967295")])
def test_ops_that_are_no_script_are_refused_after_the_launch(ctx, what, script):
    pieces = [(0, 4, 4, 0), (0, 0, 0, 0), (0, 6, 6, REV), (1, 6, 6, 0), (1, 5, 5, 0)]
    scripts = [[(SUB, 1, 1)], [], [(SUB, 0, 0)], [(SUB, 5, 5)], [(SUB, 2, 2)]]
    wrong_seg = isinstance(script, str)                       # "seg": another piece's index; "seg N": N, which is no piece's
    beyond = int(script.split()[1]) if wrong_seg and " " in script else None
    for t in (3, 2):                                          # piece 3 offends, then piece 2 as well: the smallest is named
        if not wrong_seg:
            scripts[t] = list(script)
        pc, ops, first = arrays(pieces, scripts)
        if wrong_seg:
            for u in range(t, 4):
                ops["seg"][int(first[u])] = beyond if beyond is not None else 4 if u == 3 else 0
        else:
            with pytest.raises(CB.NoScript) as err:
                CB.brute_cigar(pc.tolist(), ops.tolist(), first, 2)
            assert err.value.piece == t, what
        refused(ctx, pc, ops, first, 2, -22, f"ops of piece {t} are no script of its lengths")
    from ntsynt_amd.device import NtsError
    with pytest.raises(NtsError, match="no script"):
        ctx.cigar_build(pc, ops, first, 2)

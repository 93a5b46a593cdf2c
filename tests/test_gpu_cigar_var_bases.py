"""nts_cigar_var_bases (csrc/nts_cigar.inc, Context.cigar_var_bases; docs/design/04_32_block_variant_sites.md) over the two small uploaded
genomes of tests/test_gpu_cigar_text.py, forwards, backwards and mixed: both buffers and both firsts must equal the rows of
nts_cigar_rows (tests/maf_brute.py makes them on the CPU, and the device's own are compared as well) filtered at the X / D and X / I
columns by tests/variant_sites_brute.py; the small cases' bytes are also written out.  An X run of 9 bytes at every alignment of its
first byte, a base that is no code, chains of `=` alone (no emit launch), empty chains, 300 random chains, nts_cigar_rows' refusals with
the chain named, code 6, and the caller's four outputs untouched by a refused call.  Every expectation is computed on the CPU before the
GPU is called.  Every test runs under a time limit of its own."""
import ctypes
import faulthandler

import numpy as np
import pytest

from tests import variant_sites_brute as VB
from tests.test_gpu_cigar_rows import GOOD, case
from tests.test_gpu_cigar_text import World, random_specs

pytestmark = pytest.mark.gpu
STEP_SECONDS = 300
I, D, P, EQ, X = 1, 2, 6, 7, 8
EINVAL, ERANGE = -22, -34


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


@pytest.fixture(scope="module")
def world(ctx):
    w = World(ctx)
    yield w
    w.free()


def firsts_of(texts):
    return np.concatenate(([0], np.cumsum([len(t) for t in texts]))).astype(np.uint64)


def check(ctx, world, specs, what):
    "specs as tests/test_gpu_cigar_rows.py case's.  Returns (the chains' ref bytes, the chains' alt bytes) as strings"
    cigar, recs, spans, rows_a, rows_b = case(world, specs)
    lists = [cigar[int(r["first"]):int(r["first"] + r["n_cig"])].tolist() for r in recs]
    want = [VB.variant_bytes(entries, a, b) for entries, a, b in zip(lists, rows_a, rows_b)]
    refs, alts = [w[0] for w in want], [w[1] for w in want]
    assert [(len(r), len(a)) for r, a in want] == [VB.byte_counts(entries) for entries in lists]
    ref, ref_first, alt, alt_first = ctx.cigar_var_bases(cigar, recs, spans, *world.genomes)
    print(f"{what}: {cigar.size} entries, {recs.size} chains, {ref.size} ref and {alt.size} alt bytes")
    assert ref.dtype == np.uint8 and alt.dtype == np.uint8 and ref_first.dtype == np.uint64 and alt_first.dtype == np.uint64, what
    assert np.array_equal(ref_first, firsts_of(refs)) and np.array_equal(alt_first, firsts_of(alts)), (what, ref_first[:8], alt_first[:8])
    for name, got, texts in (("ref", ref, refs), ("alt", alt, alts)):
        have, whole = got.tobytes().decode("latin-1"), "".join(texts)
        if have != whole:
            at = next(i for i in range(min(len(have), len(whole)) + 1) if have[i:i + 1] != whole[i:i + 1])
            raise AssertionError((what, name, "first difference at byte", at, have[max(at - 12, 0):at + 12], whole[max(at - 12, 0):at + 12]))
        assert "?" not in have and "\0" not in have and "-" not in have, (what, name)
    again = ctx.cigar_var_bases(cigar, recs, spans, *world.genomes)
    assert all(x.tobytes() == y.tobytes() for x, y in zip((ref, ref_first, alt, alt_first), again)), what
    return refs, alts


def both_strands(ctx, world, specs, what):
    out = [check(ctx, world, [s + (back,) for s in specs], f"{what}, {'backwards' if back else 'forwards'}") for back in (False, True)]
    check(ctx, world, [s + (bool(c % 2),) for c, s in enumerate(specs)], what + ", mixed")
    return out


def complement(text):
    return text.translate(str.maketrans("ACGTN", "TGCAN"))


# ---- the small cases: the bytes are also written out from the genomes' strings ----

def test_the_small_cases(ctx, world):
    a, b = world.seqs[0][0], world.seqs[1][0]
    (refs, alts), (refs_back, alts_back) = both_strands(ctx, world, [("5=1X2D3=", 0, 100, 0, 200)], "5= 1X 2D 3=")
    assert refs == [a[105:108]] == refs_back and alts == [b[205]]
    assert alts_back == [complement(b[200:209][::-1])[5]]                                     # (the query's 9 bases read backwards: column 5)
    (refs, alts), (_, alts_back) = both_strands(ctx, world, [("4=2I4=", 0, 10, 0, 20)], "4= 2I 4=")
    assert refs == [""] and alts == [b[24:26]] and alts_back == [complement(b[20:30][::-1])[4:6]]
    (refs, alts), _ = both_strands(ctx, world, [([3 << 4 | X, 2 << 4 | X], 0, 50, 0, 60)], "3X 2X")
    assert refs == [a[50:55]] and alts == [b[60:65]]


def test_chains_of_equal_alone_launch_no_emit_kernel(ctx, world):
    check(ctx, world, [("5=1X2D3=", 0, 100, 0, 200, False)], "a first call")
    emits, scans = ctx.timing("cigar_var_bases_emit")[1], ctx.timing("cigar_var_bases_scan")[1]
    assert emits > 0 and scans > 0
    refs, alts = check(ctx, world, [("9=", 0, 3, 0, 4, False), ([], 0, 0, 0, 0, False), ("120=", 1, 0, 1, 7, True)], "= alone")
    assert refs == ["", "", ""] == alts
    assert ctx.timing("cigar_var_bases_emit")[1] == emits and ctx.timing("cigar_var_bases_scan")[1] == scans + 2, "scanned twice, nothing emitted"
    got = ctx.cigar_var_bases(np.zeros(0, dtype=np.uint64), case(world, [])[1], case(world, [])[2], *world.genomes)
    assert got[0].size == 0 and got[2].size == 0 and got[1].tolist() == [0] == got[3].tolist()
    assert ctx.timing("cigar_var_bases_scan")[1] == scans + 2, "no entry: nothing is launched"
    only_ref, only_alt = check(ctx, world, [("2=3D2=", 0, 5, 0, 5, False)], "ref bytes alone"), check(ctx, world, [("2=3I2=", 0, 5, 0, 5, True)], "alt bytes alone")
    assert only_ref[1] == [""] and only_alt[0] == [""] and len(only_ref[0][0]) == 3 == len(only_alt[1][0])


def test_empty_chains_first_in_the_middle_and_last(ctx, world):
    specs = [([], 0, 0, 0, 0), ("2=1X1=", 0, 10, 0, 10), ([], 1, 5, 1, 5), ([], 0, 7, 0, 7), ("1X2D3I1=", 1, 20, 1, 30), ("3=", 0, 0, 0, 0), ([], 0, 2100, 0, 2300)]
    (refs, alts), _ = both_strands(ctx, world, specs, "empty chains")
    assert [len(r) for r in refs] == [0, 1, 0, 0, 3, 0, 0] and [len(t) for t in alts] == [0, 1, 0, 0, 4, 0, 0]


def test_a_base_that_is_no_code(ctx, world):
    assert world.seqs[0][0][600:603] == "NNN" == world.seqs[1][0][600:603]
    (refs, alts), (_, alts_back) = both_strands(ctx, world, [("2=4X1=2D2=3I1=", 0, 597, 0, 598)], "N under X, D and I")
    assert refs[0][:4] == world.seqs[0][0][599:603] and "N" in refs[0] and "N" in alts[0] and "N" in alts_back[0]


def test_an_x_run_of_9_bytes_at_every_alignment_of_its_first_byte(ctx, world):
    for shift in range(4):
        front = [(f"1={shift}X1=", 1, 40, 1, 50)] if shift else []
        specs = front + [("3=9X2=", 0, 700, 0, 800), ("1=1X1=", 1, 100, 1, 100)]
        (refs, alts), _ = both_strands(ctx, world, specs, f"9 bytes from byte {shift}")
        assert sum(len(r) for r in refs[:len(front)]) == shift and refs[len(front)] == world.seqs[0][0][703:712] and alts[len(front)] == world.seqs[1][0][803:812]
        specs = front + [("3=4X5D2=", 0, 700, 0, 800), ("3=4X5I2=", 0, 900, 0, 1000)]         # nine ref bytes over X and D, nine alt bytes over X and I
        both_strands(ctx, world, specs, f"9 bytes of two entries from byte {shift}")


def test_300_random_chains(ctx, world):
    specs = random_specs(91, 300, 12)
    refs, alts = check(ctx, world, specs, "300 random chains")
    assert sum(len(r) for r in refs) > 1000 and sum(len(t) for t in alts) > 1000 and any(not r and t for r, t in zip(refs, alts))
    cigar, recs, spans, rows_a, rows_b = case(world, specs)                                 # against the device's own rows as well
    row_a, row_b, row_first = ctx.cigar_rows(cigar, recs, spans, *world.genomes)
    keep_a = np.repeat(np.isin(cigar & np.uint64(15), [X, D]), (cigar >> np.uint64(4)).astype(np.int64))
    keep_b = np.repeat(np.isin(cigar & np.uint64(15), [X, I]), (cigar >> np.uint64(4)).astype(np.int64))
    ref, _, alt, _ = ctx.cigar_var_bases(cigar, recs, spans, *world.genomes)
    assert np.array_equal(ref, row_a[keep_a]) and np.array_equal(alt, row_b[keep_b])


# ---- refusals ----

def refused(ctx, world, cigar, recs, spans, code, *words, counts=None, genomes="both"):
    "the call through the library itself: the return code, the message, no buffer returned and the caller's arrays untouched"
    recs, cigar = np.ascontiguousarray(recs), np.ascontiguousarray(cigar, dtype=np.uint64)
    n = counts or (cigar.size, recs.size)
    firsts = [np.full(max(recs.size, 1) + 1, 0xABABABABABABABAB, dtype=np.uint64) for _ in range(2)]
    before = firsts[0].tobytes()
    mark = 0x5A5A5A5A
    p_ref, p_alt = ctypes.c_void_p(mark), ctypes.c_void_p(mark)
    g_a = world.genomes[0].h if genomes in ("both", "a") else None
    g_b = world.genomes[1].h if genomes in ("both", "b") else None
    rc = ctx.lib.nts_cigar_var_bases(ctx.h, cigar.ctypes.data, int(n[0]), recs.ctypes.data, int(n[1]), g_a, g_b, spans.ctypes.data if spans is not None else None,
                                     ctypes.byref(p_ref), firsts[0].ctypes.data, ctypes.byref(p_alt), firsts[1].ctypes.data)
    said = ctx.lib.nts_last_error(ctx.h).decode()
    print(rc, said)
    assert rc == code and all(w in said for w in words), (rc, said, words)
    assert firsts[0].tobytes() == before == firsts[1].tobytes() and p_ref.value == mark and p_alt.value == mark
    return said


def test_refusals_before_any_launch(ctx, world):
    cigar, recs, spans, _, _ = case(world, GOOD)
    ctx.cigar_var_bases(cigar, recs, spans, *world.genomes)
    scans = ctx.timing("cigar_var_bases_scan")[1]
    for counts in ((2 ** 32, 4), (10, 2 ** 32), (2 ** 40, 2 ** 40)):                          # before any array is read: 1-element arrays
        refused(ctx, world, cigar[:1].copy(), recs[:1].copy(), spans[:1].copy(), ERANGE, "nts_cigar_var_bases", "2^32", counts=counts)
    for field, at, value, chain in (("first", 0, 1, 0), ("first", 1, 4, 1), ("n_cig", 1, 2, 2), ("n_cig", 3, 3, 3), ("first", 2, 2 ** 64 - 1, 2)):
        bad = recs.copy()
        bad[field][at] = value
        refused(ctx, world, cigar, bad, spans, EINVAL, f"nts_cigar_var_bases: chain {chain}", "do not tile")
    refused(ctx, world, cigar, recs[:0], spans[:0], EINVAL, "do not tile")                    # entries and no chain
    bad = spans.copy()
    bad["flags"][1], bad["flags"][3] = 3, 2
    refused(ctx, world, cigar, recs, bad, EINVAL, "chain 1 has unknown flag bits")
    for field in ("rec_a", "rec_b"):
        bad = spans.copy()
        bad[field][1], bad[field][3] = 3, 0xFFFFFFFF
        refused(ctx, world, cigar, recs, bad, EINVAL, "chain 1 names a record outside its genome")
    for chain, field, value in ((0, "pos_a", 2100 - 12 + 1), (0, "pos_b", 2300 - 13 + 1), (1, "pos_b", 1300), (1, "pos_b", 6), (3, "pos_b", 4), (2, "pos_b", 2301)):
        bad = spans.copy()
        bad[field][chain] = value
        bad["pos_a"][3] = max(int(bad["pos_a"][3]), 2098)                                   # (a later offender as well)
        refused(ctx, world, cigar, recs, bad, EINVAL, f"nts_cigar_var_bases: chain {chain}: its span lies outside its record")
    for which in ("a", "b", "none"):
        refused(ctx, world, cigar, recs, spans, EINVAL, "nts_cigar_var_bases", "genomes", genomes=which)
    refused(ctx, world, cigar, recs, None, EINVAL, "nts_cigar_var_bases", "spans")
    huge = recs.copy()
    huge["len_a"][0] = 2 ** 62
    refused(ctx, world, cigar, huge, spans, ERANGE, "2^62")
    assert ctx.timing("cigar_var_bases_scan")[1] == scans, "refused before any launch"
    with pytest.raises(ValueError, match="one span per chain"):
        ctx.cigar_var_bases(cigar, recs, spans[:2], *world.genomes)


def test_entries_that_are_no_cigar_and_code_6_are_refused_after_the_scan(ctx, world):
    cigar, recs, spans, _, _ = case(world, GOOD)
    emits = ctx.timing("cigar_var_bases_emit")[1]
    assert cigar.size == 10 and [int(r["first"]) for r in recs] == [0, 5, 8, 8]
    for at, value, chain in ((3, 1 << 4 | 3, 0), (7, 2 << 4 | 0, 1), (6, 0 << 4 | I, 1), (9, 7 << 4 | 15, 3), (1, 1 << 4 | P, 0), (8, 4 << 4 | P, 3)):
        bad = cigar.copy()
        bad[9] = 7 << 4 | 15                                 # (a later offender as well: the smallest chain is named)
        bad[at] = value
        refused(ctx, world, bad, recs, spans, EINVAL, f"nts_cigar_var_bases: the entries of chain {chain} are no CIGAR of its lengths")
    for field in ("len_a", "len_b"):                          # lengths that disagree with the entries
        off = recs.copy()
        off[field][1] = int(off[field][1]) - 1
        off["len_a"][3] -= 1
        refused(ctx, world, cigar, off, spans, EINVAL, "the entries of chain 1 are no CIGAR of its lengths")
    assert ctx.timing("cigar_var_bases_emit")[1] == emits
    check(ctx, world, GOOD, "the context still answers")

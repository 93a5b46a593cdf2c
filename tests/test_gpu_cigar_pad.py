"""nts_cigar_pad and nts_cigar_rows_padded (csrc/nts_cigar.inc, Context.cigar_pad, Context.cigar_rows(padded=True);
docs/design/04_30_block_maf_multi.md) against tests/multi_maf_brute.py: padded entries, pad_first and the sites of hand-made groups -- the
smallest shapes that can go wrong -- and the padded rows of the same groups over the two small genomes of tests/test_gpu_cigar_text.py,
forwards and backwards.  Every expectation is computed on the CPU before the GPU is called.  Every test runs under a time limit of its
own."""
import faulthandler

import numpy as np
import pytest

from tests import multi_maf_brute as MM
from tests.test_gpu_cigar_lift import arrays
from tests.test_gpu_cigar_text import World

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


def at_of(specs):
    from ntsynt_amd.device import CIG_PAD_AT_DTYPE
    at = np.zeros(len(specs), dtype=CIG_PAD_AT_DTYPE)
    for c, (group, t0, _) in enumerate(specs):
        at[c] = (group, 0, t0)
    return at


def check(ctx, specs, what, n_groups=None):
    "specs: per chain (group, t0, CIGAR string or entries).  Returns (the brute force's lists, the entry lists of the chains)"
    cigar, recs, lists = arrays([s[2] for s in specs])
    chains = [(g, t0, lists[c]) for c, (g, t0, _) in enumerate(specs)]
    groups = n_groups if n_groups is not None else (specs[-1][0] + 1 if specs else 0)
    want = MM.pad_all(chains, groups)
    got = ctx.cigar_pad(cigar, recs, at_of(specs), n_groups)
    print(f"{what}: {cigar.size} entries, {recs.size} chains, {groups} groups -> {got[0].size} entries, {got[3].size} sites")
    assert len(got) == 5 and all(x.dtype == np.uint64 for x in got), what
    for name, have, exp in zip(("padded", "pad_first", "site_first", "site_pos", "site_w"), got, want):
        if have.tolist() != list(exp):
            at = next(i for i in range(max(len(have), len(exp))) if have[i:i + 1].tolist() != list(exp[i:i + 1]))
            raise AssertionError((what, name, "first difference at", at, have[max(at - 3, 0):at + 4].tolist(), list(exp[max(at - 3, 0):at + 4])))
    again = ctx.cigar_pad(cigar, recs, at_of(specs), n_groups)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), what
    return want, lists


def text_of(entries):
    return "".join(f"{int(v) >> 4}{'?ID???P=X'[int(v) & 15]}" for v in entries)


def chain_texts(want):
    padded, first = want[0], want[1]
    return [text_of(padded[first[c]:first[c + 1]]) for c in range(len(first) - 1)]


# ---- hand-made groups: the expectation is also written out, so that the brute force is checked too ----

def test_two_insertions_of_3_and_5_in_one_slot(ctx):
    want, _ = check(ctx, [(0, 100, "4=3I4="), (0, 100, "4=5I4=")], "I 3 and I 5 in one slot")
    assert chain_texts(want) == ["4=3I2P4=", "4=5I4="] and want[3:] == ([104], [5])


def test_a_foreign_site_inside_a_run_and_at_run_boundaries(ctx):
    specs = [(0, 10, "10=2I10="),          # the site: slot 20, width 2
             (0, 10, "20="),               # strictly inside an = run
             (0, 10, "10=10X"),            # at an = / X boundary
             (0, 10, "10=5D5="),           # at an = / D boundary
             (0, 10, "5=10D5="),           # inside a D run
             (0, 5, "15X5=")]              # at an X / = boundary of a chain that begins elsewhere
    want, _ = check(ctx, specs, "foreign sites")
    assert chain_texts(want) == ["10=2I10=", "10=2P10=", "10=2P10X", "10=2P5D5=", "5=5D2P5D5=", "15X2P5="]


def test_an_own_insertion_directly_followed_by_a_deletion(ctx):
    want, _ = check(ctx, [(0, 0, "5=2I3D5="), (0, 0, "5=4I8="), (0, 0, "13=")], "own I followed by D")
    assert chain_texts(want) == ["5=2I2P3D5=", "5=4I8=", "5=4P8="]


def test_a_site_at_another_chains_t0_and_t1(ctx):
    specs = [(0, 0, "10=3I10="),           # site at slot 10
             (0, 10, "8="),                # begins at the site: a leading P
             (0, 2, "8="),                 # ends at the site: nothing
             (0, 10, "1X"),                # one base behind the site
             (0, 9, "1X")]                 # one base in front of it
    want, _ = check(ctx, specs, "sites at t0 and t1")
    assert chain_texts(want) == ["10=3I10=", "3P8=", "8=", "3P1X", "1X"]


def test_a_chain_no_site_touches_and_groups_with_equal_slots(ctx):
    specs = [(0, 50, "10=1I10="), (0, 0, "40="),             # group 0: the second chain lies in front of the site
             (1, 50, "21="), (1, 50, "30=6I1="),               # group 1: the same reference bases, a site of its own at slot 80
             (3, 50, "21=")]                                  # group 2 has no chain; group 3 has no site
    want, lists = check(ctx, specs, "untouched chains, equal slots in two groups")
    assert chain_texts(want) == ["10=1I10=", "40=", "21=", "30=6I1=", "21="]
    assert want[2] == [0, 1, 2, 2, 2] and want[3] == [60, 80] and want[4] == [1, 6]
    assert want[0] == [v for entries in lists for v in entries]


def test_empty_chains_between_non_empty_ones(ctx):
    specs = [(0, 0, ""), (0, 0, "6=2I6="), (0, 3, ""), (0, 0, ""), (0, 0, "12="), (1, 7, ""), (1, 0, "3=1I3="), (1, 0, "")]
    want, _ = check(ctx, specs, "empty chains")
    assert chain_texts(want) == ["", "6=2I6=", "", "", "6=2P6=", "", "3=1I3=", ""]
    check(ctx, [(0, 5, ""), (0, 6, "")], "only empty chains")


def test_one_group_of_one_chain_and_no_chain_at_all(ctx):
    want, _ = check(ctx, [(0, 7, "3=2I1X4D2=1I1=")], "one group of one chain")
    assert chain_texts(want) == ["3=2I1X4D2=1I1="] and want[3] == [10, 17]
    before = ctx.timing("cigar_pad_sites")[1], ctx.timing("cigar_pad_emit")[1]
    got = ctx.cigar_pad(np.zeros(0, dtype=np.uint64), arrays([])[1], at_of([]), 0)
    assert [x.tolist() for x in got] == [[], [0], [0], [], []]
    got = ctx.cigar_pad(np.zeros(0, dtype=np.uint64), arrays([])[1], at_of([]), 3)
    assert [x.tolist() for x in got] == [[], [0], [0, 0, 0, 0], [], []]
    assert (ctx.timing("cigar_pad_sites")[1], ctx.timing("cigar_pad_emit")[1]) == before, "no chain: nothing is launched"


def test_a_run_crossed_by_600_foreign_sites(ctx):
    "one = entry becomes 1 201 entries: more than two workgroups of output lanes for one input entry"
    specs = [(0, 1000, "20000=")]
    specs += [(0, 1000 + 30 * j, f"10={1 + j % 7}I10=") for j in range(600)]
    want, _ = check(ctx, specs, "600 foreign sites in one run")
    assert want[1][1] == 1201 and len(want[3]) == 600
    specs[0] = (0, 1000, "7000=12990D10=")                    # (the first 233 sites split the = run, the others the D run)
    check(ctx, specs, "600 foreign sites in two runs")


def random_groups(seed, n_chains, n_groups):
    rng = np.random.default_rng(seed)
    groups = np.sort(rng.integers(0, n_groups, n_chains))
    specs = []
    for g in groups:
        entries = []
        if rng.integers(0, 12):                               # (one chain in twelve is empty)
            for k in range(int(rng.integers(1, 14))):
                code = int(rng.choice([EQ, EQ, X, I, D])) if k else EQ
                if entries and entries[-1] & 15 == code:
                    code = EQ if code != EQ else X
                entries.append(int(rng.integers(1, 9)) << 4 | code)
            entries.append(int(rng.integers(1, 6)) << 4 | (X if entries[-1] & 15 == EQ else EQ))
        specs.append((int(g), int(rng.integers(0, 40)) + (1 << 33) * (int(g) % 2), entries))   # (odd groups beyond 2^32: t0 is 64 bits wide)
    return specs


def test_300_random_chains_in_40_groups(ctx):
    specs = random_groups(5, 300, 40)
    want, _ = check(ctx, specs, "300 random chains", n_groups=40)
    assert len(want[3]) > 100 and any(v & 15 == P for v in want[0]) and len(want[0]) > sum(len(s[2]) for s in specs)
    check(ctx, random_groups(6, 300, 40), "300 other random chains", n_groups=40)


# ---- refusals ----

def refused(ctx, specs, code, words, n_groups=None, mutate=None):
    from ntsynt_amd.device import NtsError
    cigar, recs, _ = arrays([s[2] for s in specs])
    if mutate:
        mutate(cigar, recs)
    with pytest.raises(NtsError) as err:
        ctx.cigar_pad(cigar, recs, at_of(specs), n_groups)
    assert f"(code {code})" in str(err.value) and all(w in str(err.value) for w in words), (code, words, str(err.value))


def test_refusals_name_the_smallest_offending_chain(ctx):
    good = (0, 0, "4=1I4=")
    refused(ctx, [good, (1, 0, "4="), (0, 0, "4="), (0, 0, "1I4=")], EINVAL, ["chain 2", "nondecreasing"], n_groups=2)
    refused(ctx, [good, (0, 0, "2I4="), (0, 0, "4=1D")], EINVAL, ["chain 1", "not = or X"])
    refused(ctx, [good, (0, 0, "4=2D")], EINVAL, ["chain 1", "not = or X"])
    refused(ctx, [good, (0, 0, "1D")], EINVAL, ["chain 1", "not = or X"])
    refused(ctx, [good, good, (2, 0, "4=")], EINVAL, ["chain 2", "n_groups"], n_groups=2)
    refused(ctx, [good, (0, 0, [4 << 4 | EQ, 2 << 4 | P, 4 << 4 | EQ]), (0, 0, [1 << 4 | EQ, 1 << 4 | P, 1 << 4 | X])], EINVAL, ["chain 1", "code 6"])
    refused(ctx, [good, (0, 0, [4 << 4 | EQ, 2 << 4 | 3, 4 << 4 | EQ])], EINVAL, ["chain 1", "no CIGAR of its lengths"])
    refused(ctx, [good, (0, 0, [4 << 4 | EQ, 0 << 4 | D, 4 << 4 | EQ])], EINVAL, ["chain 1", "no CIGAR of its lengths"])
    refused(ctx, [good, (0, 1 << 32, "4=")], ERANGE, ["chain 1", "2^32"])
    refused(ctx, [good, (0, (1 << 64) - 2, "4=")], ERANGE, ["chain 1", "wraps"])

    def long(cigar, recs):
        recs["len_a"][1] = 1 << 62
    refused(ctx, [good, (0, 0, "4=")], ERANGE, ["2^62 bases or more"], mutate=long)

    def shift(cigar, recs):
        recs["first"][1] += 1
    refused(ctx, [good, (0, 0, "4=")], EINVAL, ["chain 1", "tile"], mutate=shift)
    want, _ = check(ctx, [good, (0, (1 << 32) - 9, "4=")], "an extent of 2^32 - 1 - 4 bases passes")   # (t1 = 2^32 - 5)
    assert chain_texts(want) == ["4=1I4=", "4="]


# ---- the padded rows ----

def rows_case(world, specs, back):
    """specs: per chain (group, t0, CIGAR) -- every chain reads target record 0 at t0 and query record 0, chain c at 40 c.  Returns what
    cigar_rows needs for the padded chains and the brute force's rows"""
    from ntsynt_amd.device import CIG_B_BACKWARDS, CIG_SPAN_DTYPE
    _, _, lists = arrays([s[2] for s in specs])
    padded, first = MM.pad_all([(g, t0, lists[c]) for c, (g, t0, _) in enumerate(specs)], specs[-1][0] + 1)[:2]
    pieces = [padded[first[c]:first[c + 1]] for c in range(len(specs))]
    recs = arrays([[v for v in p if v & 15 != P] for p in pieces])[1]      # the totals of the unpadded chain ...
    at = 0
    for c, p in enumerate(pieces):                                        # ... over the padded entries
        recs[c]["first"], recs[c]["n_cig"] = at, len(p)
        at += len(p)
    spans = np.zeros(len(specs), dtype=CIG_SPAN_DTYPE)
    rows = []
    for c, (g, t0, _) in enumerate(specs):
        la, lb, sb = MM.len_a(lists[c]), MM.len_b(lists[c]), 40 * c
        target, query = world.seqs[0][0][t0:t0 + la], world.seqs[1][0][sb:sb + lb]
        assert len(target) == la and len(query) == lb
        spans[c] = (t0, sb + lb - 1 if back and lb else sb, 0, 0, CIG_B_BACKWARDS if back else 0, 0)
        rows.append(MM.padded_rows(pieces[c], MM.letters(target), MM.reverse_complement(query) if back else MM.letters(query)))
    return np.array([v for p in pieces for v in p], dtype=np.uint64), recs, spans, rows


ROW_GROUPS = [(0, 10, "10=2I10="), (0, 10, "20="), (0, 10, "10=10X"), (0, 10, "10=5D5="), (0, 5, "5=10D5=1I5="), (0, 5, "15X5="), (0, 20, "3="),
              (0, 0, ""), (1, 590, "8=3I2D9="), (1, 595, "3=5I20="), (1, 580, "30=")]     # (group 1 crosses the N at bases 600 .. 602)


@pytest.mark.parametrize("back", [False, True], ids=["forwards", "backwards"])
def test_padded_rows_match_the_brute_force(ctx, world, back):
    cigar, recs, spans, rows = rows_case(world, ROW_GROUPS, back)
    assert any(int(v) & 15 == P for v in cigar)
    row_a, row_b, first = ctx.cigar_rows(cigar, recs, spans, *world.genomes, padded=True)
    have_a, have_b = row_a.tobytes().decode("latin-1"), row_b.tobytes().decode("latin-1")
    assert first.tolist() == np.concatenate(([0], np.cumsum([len(a) for a, _ in rows]))).tolist()
    assert have_a == "".join(a for a, _ in rows) and have_b == "".join(b for _, b in rows)
    assert not set(have_a + have_b) - set("ACGTN-"), "no ? and no 0 byte"
    sites = MM.widths([(g, t0, arrays([s])[2][0]) for g, t0, s in ROW_GROUPS])
    for c, (g, t0, s) in enumerate(ROW_GROUPS):               # every chain has col0(t1) - col0(t0) columns
        t1 = t0 + MM.len_a(arrays([s])[2][0])
        r0 = min(t for gg, t, _ in ROW_GROUPS if gg == g)
        assert int(first[c + 1] - first[c]) == MM.col0(r0, sites[g], t1) - MM.col0(r0, sites[g], t0), c


def test_rows_without_the_flag_refuse_code_6_and_keep_their_bytes(ctx, world):
    from ntsynt_amd.device import NtsError
    cigar, recs, spans, rows = rows_case(world, ROW_GROUPS, False)
    with pytest.raises(NtsError) as err:
        ctx.cigar_rows(cigar, recs, spans, *world.genomes)
    assert f"(code {EINVAL})" in str(err.value) and "nts_cigar_rows:" in str(err.value) and "no CIGAR of its lengths" in str(err.value)
    plain = [s for s in ROW_GROUPS if s[2] in ("20=", "10=10X", "10=5D5=")]
    cigar, recs, spans, rows = rows_case(world, [(g, t0, s) for g, t0, s in [(0, 10, "10=2I10=")] + plain][1:], True)
    assert not any(int(v) & 15 == P for v in cigar)           # (no site among them: unpadded input)
    without, padded = ctx.cigar_rows(cigar, recs, spans, *world.genomes), ctx.cigar_rows(cigar, recs, spans, *world.genomes, padded=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(without, padded))
    assert without[0].tobytes().decode() == "".join(a for a, _ in rows) and without[1].tobytes().decode() == "".join(b for _, b in rows)

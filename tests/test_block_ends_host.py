"""The host side of the block ends (ntsynt_amd/assess.py check_ends_parameters, ends_tasks, ends_stop, ends_row, ends_table;
docs/design/04_20_block_ends.md) on hand-made rounds, no GPU: the device call is stood in for by tests/extend_brute.py reading the
tasks' strings from the records, and every pair's columns are compared with that module's own recomputation, which works a flipped
pair in the frame of the whole record's reverse complement.  `+` and `-` pairs, an interval without an aligned segment, a first and a
last segment that are not aligned, flank lengths clipped by the record's start, its end and max_len, every stop reason and the
precedence among them, the file's header, `.` line and footer."""
import numpy as np
import pytest

from ntsynt_amd import assess
from ntsynt_amd.device import EDIT_INVALID, EDIT_OVERBAND, EDIT_PASSED, EXTEND_DTYPE, SEGMENT_DTYPE, TASK_DTYPE
from tests import extend_brute as X

LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)
PENALTY, MAX_EDITS = 6, 40


def dna(rng, n):
    return LETTERS[rng.integers(0, 4, size=n)]


def mutated(rng, s, rate):
    out = s.copy()
    for at in np.flatnonzero(rng.random(s.size) < rate):
        out[at] = rng.choice(LETTERS[LETTERS != out[at]])
    return out


class Line:
    def __init__(self, block_id, genome, contig, strand):
        self.block_id, self.genome, self.contig, self.strand = block_id, genome, contig, strand


def world(seed=5):
    """genome A: one record of 3 000 bases and a second one; genome B: record 0 a 1 % copy of A's record 0 behind 23 other bases, record 1
    its reverse complement between 11 and 37 other bases.  The interval of A is [500, 2500); its mates are where B holds those bases."""
    rng = np.random.default_rng(seed)
    a0 = dna(rng, 3000)
    copy = mutated(rng, a0, 0.01)
    copy[2300:2420] = dna(rng, 120)                           # (unrelated from 2300 on for a while: a break inside the right flank)
    rec_a = [a0, dna(rng, 50)]
    rec_b = [np.concatenate([dna(rng, 23), copy]), np.concatenate([dna(rng, 11), X.revcomp(copy), dna(rng, 37)])]
    iv_a = (0, 500, 2500)
    iv_b = {False: (0, 523, 2523), True: (1, 11 + 3000 - 2500, 11 + 3000 - 500)}
    return rec_a, rec_b, iv_a, iv_b


def segments(rows):
    arr = np.zeros(len(rows), dtype=SEGMENT_DTYPE)
    for q, row in enumerate(rows):
        arr[q] = row
    return arr


def device_stand_in(rec_a, rec_b, tasks, penalty, max_edits):
    "what nts_edit_extend returns, by the brute force over the tasks' strings"
    out = np.zeros(tasks.size, dtype=EXTEND_DTYPE)
    for q, t in enumerate(tasks):
        out[q] = X.extend_brute(*X.task_strings(rec_a, rec_b, (t["rec_a"], t["pos_a"], t["n"], t["rec_b"], t["pos_b"], t["m"], t["flags"])),
                                penalty, max_edits)[0]
    return out


SEGS = [(0, 100, 200, 100, 200, 0), (0, 300, 400, 300, 400, 0), (0, 700, 1000, 700, 1000, 0)]


@pytest.mark.parametrize("flipped", [False, True])
@pytest.mark.parametrize("final,max_len", [([3, 4, 9], 4096), ([3, 4, 9], 250), ([EDIT_OVERBAND, 4, 9], 4096), ([3, 4, EDIT_INVALID], 4096),
                                           ([EDIT_PASSED, 0, EDIT_OVERBAND], 700)])
def test_tasks_and_rows_against_the_recomputation(flipped, final, max_len):
    rec_a, rec_b, iv_a, iv_b = world()
    segs = segments(SEGS)
    ivs_a, ivs_b = np.array([iv_a], dtype=np.uint64), np.array([iv_b[flipped]], dtype=np.uint64)
    tasks, flanks = assess.ends_tasks(segs, np.array(final, dtype=np.uint32), ivs_a, ivs_b, [int(flipped)], [(0, 1, 0)], [r.size for r in rec_a],
                                      [r.size for r in rec_b], max_len)
    assert tasks.dtype == TASK_DTYPE and tasks.size == 2 and flanks[0]["left"] == 0 and flanks[0]["right"] == 1
    aligned = [s for s, d in zip(SEGS, final) if d < EDIT_INVALID]
    assert (flanks[0]["x_l"], flanks[0]["x_r"]) == (aligned[0][1], aligned[-1][1] + aligned[-1][2])      # (an end point moves inwards)
    # the lengths asked for: clipped by the record's start, by its end and by max_len
    left, right = tasks[0], tasks[1]
    assert left["n"] == min(max_len, 500 + flanks[0]["x_l"]) and right["n"] == min(max_len, 3000 - 500 - flanks[0]["x_r"])
    b_before, b_behind = (23, 0) if not flipped else (37, 11)     # what B's record holds in front of and behind the copy, oriented
    assert left["m"] == min(max_len, b_before + 500 + flanks[0]["y_l"]) and right["m"] == min(max_len, 3000 - 500 - flanks[0]["y_r"] + b_behind)
    results = device_stand_in(rec_a, rec_b, tasks, PENALTY, MAX_EDITS)
    la, lb = Line("7", "a.fa", "chr1", "+"), Line("7", "b.fa", "chr9", "-" if flipped else "+")
    row = assess.ends_row(la, lb, ivs_a[0], ivs_b[0], flipped, flanks[0], tasks, results, max_len, MAX_EDITS)
    want = X.pair_ends(rec_a[0], rec_b[int(flipped)], (500, 2000), (int(ivs_b[0][1]), 2000), flipped, list(zip(SEGS, final)), max_len, MAX_EDITS,
                       PENALTY)
    assert {c: row[c] for c in want} == want, (row, want)
    assert [row[c] for c in assess.ENDS_COLUMNS[:10]] == ["7", "a.fa", "chr1", 500, 2500, "b.fa", "chr9", int(ivs_b[0][1]), int(ivs_b[0][2]),
                                                          "-" if flipped else "+"]
    # what the world was made for: the left flank reaches the record's start in A unless max_len is shorter; the right one breaks at 2300
    assert row["left_stop"] == ("record" if max_len > 500 + flanks[0]["x_l"] else "max_len")
    if flanks[0]["x_r"] == 1700:
        assert row["right_stop"] == "break" and abs(row["ext_end_a"] - 2300) <= 16


def test_a_pair_without_an_aligned_segment_has_no_flanks():
    rec_a, rec_b, iv_a, iv_b = world()
    segs = segments(SEGS + [(1, 5, 10, 5, 10, 0)])
    ivs_a, ivs_b = np.array([iv_a, iv_a, iv_a], dtype=np.uint64), np.array([iv_b[False], iv_b[False], iv_b[True]], dtype=np.uint64)
    final = np.array([EDIT_PASSED, EDIT_OVERBAND, EDIT_INVALID, 2], dtype=np.uint32)
    lines = [(0, 3, 0), (1, 4, 1), (2, 5, 2)]                 # interval 0: nothing aligned; 1: one segment; 2: no segment at all
    tasks, flanks = assess.ends_tasks(segs, final, ivs_a, ivs_b, [0, 0, 1], lines, [3000, 50], [3023, 3048], 100)
    assert flanks[0] is None and flanks[2] is None and tasks.size == 2 and (flanks[1]["x_l"], flanks[1]["x_r"], flanks[1]["left"]) == (5, 15, 0)
    row = assess.ends_row(Line("1", "a", "c", "+"), Line("1", "b", "d", "+"), ivs_a[0], ivs_b[0], False, None, tasks, None, 100, 9)
    assert [row[c] for c in assess.ENDS_COLUMNS[10:]] == ["."] * 12 and row["start_b"] == 523
    text = assess.ends_table([row], 21, 16, 31, 4096, 0, 100, 9, 6)
    assert text.splitlines() == ["\t".join(assess.ENDS_COLUMNS), "1\ta\tc\t500\t2500\tb\td\t523\t2523\t+" + "\t." * 12,
                                 "# k 21, rate 16, band 31, max_len 4096, max_edits 0, ends_max_len 100, ends_max_edits 9, ends_penalty 6"]


def test_an_end_point_at_the_record_s_first_or_last_base_asks_for_no_base():
    rec_a, rec_b, _, _ = world()
    segs = segments([(0, 0, 3000, 0, 3000, 0)])
    for flipped, iv_b in ((False, (0, 23, 3023)), (True, (1, 11, 3011))):
        tasks, flanks = assess.ends_tasks(segs, np.array([30], dtype=np.uint32), np.array([(0, 0, 3000)], dtype=np.uint64),
                                          np.array([iv_b], dtype=np.uint64), [int(flipped)], [(0, 1, 0)], [3000, 50], [3023, 3048], 4096)
        assert (tasks["n"].tolist(), tasks["m"].tolist()) == ([0, 0], [37, 11] if flipped else [23, 0])
        assert tasks["pos_a"].tolist() == [0, 0] and all(int(t["pos_b"]) <= rec_b[int(flipped)].size for t in tasks)
        results = device_stand_in(rec_a, rec_b, tasks, PENALTY, MAX_EDITS)
        row = assess.ends_row(Line("1", "a", "c", "+"), Line("1", "b", "d", "-" if flipped else "+"), (0, 0, 3000), iv_b, flipped, flanks[0], tasks,
                              results, 4096, MAX_EDITS)
        assert (row["left_stop"], row["right_stop"], row["ext_start_a"], row["ext_end_a"]) == ("record", "record", 0, 3000)
        assert (row["ext_start_b"], row["ext_end_b"]) == (iv_b[1], iv_b[2])


def test_every_stop_reason_and_the_precedence_among_them():
    def stop(ext_a, ext_b, edits, valid_a, valid_b, n, m, max_len=100, max_edits=9):
        return assess.ends_stop({"n": n, "m": m}, {"ext_a": ext_a, "ext_b": ext_b, "edits": edits, "valid_a": valid_a, "valid_b": valid_b}, max_len, max_edits)
    assert stop(50, 40, 2, 60, 60, 60, 60) == "break"
    assert stop(50, 40, 9, 60, 60, 60, 60) == "max_edits"
    assert stop(60, 40, 2, 60, 70, 60, 70) == "record" and stop(100, 40, 2, 100, 70, 100, 70) == "max_len" and stop(60, 40, 2, 60, 70, 80, 70) == "invalid"
    assert stop(40, 70, 2, 80, 70, 80, 70) == "record" and stop(40, 100, 2, 80, 100, 80, 100) == "max_len" and stop(40, 70, 2, 80, 70, 80, 90) == "invalid"
    # a limit kind: invalid before max_len (a string of max_len bases that was cut); A's before B's; either before max_edits
    assert stop(60, 40, 2, 60, 70, 100, 70) == "invalid"
    assert stop(60, 70, 9, 60, 70, 60, 100) == "record" and stop(100, 70, 9, 100, 70, 100, 90) == "max_len"
    assert stop(40, 70, 9, 80, 70, 80, 90) == "invalid" and stop(0, 0, 0, 0, 0, 0, 0) == "record" and stop(0, 0, 0, 0, 5, 3, 5) == "invalid"


def test_parameter_messages():
    assert assess.check_ends_parameters(assess.ENDS_MAX_LEN, assess.ENDS_MAX_EDITS, assess.ENDS_PENALTY) is None
    assert assess.check_ends_parameters(1, 1, 3) is None and assess.check_ends_parameters(65535, 1023, 255) is None
    for bad, word in (((0, 255, 6), "--ends-max-len"), ((65536, 255, 6), "--ends-max-len"), ((4096, 0, 6), "--ends-max-edits"),
                      ((4096, 1024, 6), "--ends-max-edits"), ((4096, 255, 2), "--ends-penalty"), ((4096, 255, 256), "--ends-penalty")):
        assert word in assess.check_ends_parameters(*bad), bad
    with pytest.raises(ValueError, match="--ends-penalty"):
        assess.block_ends(None, {}, [], ends_penalty=2)
    with pytest.raises(ValueError, match="--identity-band"):
        assess.block_ends(None, {}, [], band=32)


def test_the_pipeline_refuses_what_the_switch_refuses():
    from ntsynt_amd import pipeline
    for bad in ((4096, 255), (4096, 255, 2), (4096, 255, 6, 21, 16, 32, 4096), (0, 255, 6)):
        with pytest.raises(ValueError, match="block_ends"):
            pipeline.run(["a.fa", "b.fa"], block_ends=bad, backend=object())

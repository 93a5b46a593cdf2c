"""Gap copy sites by their definitions, over dictionaries (docs/design/04_13_gap_copy_sites.md): what tests/test_gpu_iv_sites.py holds
nts_iv_sites against and what tests/test_gpu_gap_copy_sites.py recomputes the file from.  No GPU, nothing of ntsynt_amd/gaps.py's
copy_sites."""
from collections import defaultdict

import numpy as np

SAMPLE = np.dtype([("h0", "<u8"), ("iv", "<u4"), ("off", "<u4")])


def samples(rows):
    "[(hash, iv, off)] as nts_sample records"
    out = np.zeros(len(rows), dtype=SAMPLE)
    for i, (h, iv, off) in enumerate(rows):
        out[i] = (h, iv, off)
    return out


def gap_sites(pairs, step):
    """the sites of one gap in one target: pairs = [(o.rec, o.pos, q's index in its list, q.off)], any order.  Ordered by (o.rec, o.pos,
    q's index), a site is a maximal run of consecutive pairs with equal o.rec whose consecutive o.pos differ by at most step.  Returns
    [(rec, hits, fwd, rev, min q.off, max q.off, smallest o.pos, largest o.pos)] in (rec, smallest o.pos) order."""
    out, run = [], []

    def close():
        offs = [p[3] for p in run]
        fwd = sum(b > a for a, b in zip(offs, offs[1:]))
        rev = sum(b < a for a, b in zip(offs, offs[1:]))
        out.append((run[0][0], len(run), fwd, rev, min(offs), max(offs), run[0][1], run[-1][1]))
    for p in sorted(pairs, key=lambda p: (p[0], p[1], p[2])):
        if run and (p[0] != run[-1][0] or p[1] - run[-1][1] > step):
            close()
            run = []
        run.append(p)
    if run:
        close()
    return out


def brute_sites(lists, target, step, min_hits):
    """nts_iv_sites by the definitions: [(list_q, iv_q, rec_t, hits, fwd, rev, min_off_q, max_off_q, first_t, last_t)] of the sites with
    hits >= min_hits, by (list_q, iv_q, rec_t, first_t)"""
    where = defaultdict(list)                                                   # hash -> [(rec, pos)] of the target, in its order
    for h, rec, pos in zip(target["h0"].tolist(), target["iv"].tolist(), target["off"].tolist()):
        where[h].append((rec, pos))
    out = []
    for li, lst in enumerate(lists):
        pairs = defaultdict(list)                                               # gap -> its pairs
        for qi, (h, gap, off) in enumerate(zip(lst["h0"].tolist(), lst["iv"].tolist(), lst["off"].tolist())):
            for rec, pos in where.get(h, ()):
                pairs[gap].append((rec, pos, qi, off))
        for gap in sorted(pairs):
            for rec, hits, fwd, rev, lo, hi, first, last in gap_sites(pairs[gap], step):
                if hits >= min_hits:
                    out.append((li, gap, rec, hits, fwd, rev, lo, hi, first, last))
    return out

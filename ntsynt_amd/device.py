"""Host-side objects over the C ABI (include/ntsynt_hip.h): Context, Genome, BloomFilter, sketch.

Names follow the interfaces of the reference they stand in for:
  KmerBloomFilter.insert / contains-cascade / get_fpr / save   (btllib, used by
      src/ntsynt_make_common_bf.cpp:121-164)
  Indexlr-style minimize() -> minimizers per record             (btllib `indexlr`, smk:81-85)
All compute happens in libntsynt_hip.so on the GPU; there is no CPU path here."""
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import Interval, c_vp, u64


class NtsError(RuntimeError):
    pass


MEM_EVENT_NAMES = ("driver_calls", "ns_in_driver_calls", "served_from_cache", "retried_after_emptying_the_cache", "bytes_from_driver",
                   "bytes_to_driver", "ns_waiting_for_device_before_keeping_a_block", "reserve_calls")


def mem_events(lib):
    "nts_mem_events of a loaded library (no context needed: the counters are the process's)"
    out = (ctypes.c_uint64 * 8)()
    lib.nts_mem_events(out)
    return dict(zip(MEM_EVENT_NAMES, [int(x) for x in out]))


def mem_events_since(lib, before):
    "what a stage did to the allocator, in the units a bench line prints"
    now = mem_events(lib)
    d = {k: now[k] - before[k] for k in now}
    return {"hipMalloc_hipFree_calls": d["driver_calls"], "ms_in_hipMalloc_hipFree": round(d["ns_in_driver_calls"] * 1e-6, 2),
            "allocations_served_from_kept_memory": d["served_from_cache"], "allocations_retried_after_emptying_the_cache": d["retried_after_emptying_the_cache"],
            "GB_from_driver": round(d["bytes_from_driver"] / 1e9, 3), "GB_to_driver": round(d["bytes_to_driver"] / 1e9, 3),
            "ms_waiting_for_device_before_keeping_a_block": round(d["ns_waiting_for_device_before_keeping_a_block"] * 1e-6, 2),
            "reserve_calls": d["reserve_calls"]}


# nts_sample / nts_iv_link (include/ntsynt_hip.h) as numpy records: what Genome.bf_sample_intervals returns and Context.iv_links joins
SAMPLE_DTYPE = np.dtype([("h0", "<u8"), ("iv", "<u4"), ("off", "<u4")])
LINK_DTYPE = np.dtype([(n, "<u4") for n in ("list_a", "iv_a", "list_b", "iv_b", "anchors", "fwd", "rev", "min_off_a", "max_off_a", "min_off_b",
                                            "max_off_b")])
# nts_iv_site: what Context.iv_sites returns
SITE_DTYPE = np.dtype([(n, "<u4") for n in ("list_q", "iv_q", "rec_t", "hits", "fwd", "rev", "min_off_q", "max_off_q", "first_t", "last_t")])
# nts_iv_period: what Context.iv_periods returns, one per interval
PERIOD_DTYPE = np.dtype([(n, "<u4") for n in ("recurring", "period", "period_hits", "first_off", "last_off")])
# nts_iv_fsite: what Context.iv_family_sites returns
FSITE_DTYPE = np.dtype([(n, "<u4") for n in ("family", "rec", "first", "last", "hits")])
# nts_iv_segment / nts_iv_identity: what Context.iv_anchor_segments and Context.edit_segments return
SEGMENT_DTYPE = np.dtype([("iv_a", "<u4"), ("x", "<u4"), ("dx", "<u4"), ("y_lo", "<u4"), ("dy", "<i4"), ("kind", "<u4")])
IDENTITY_DTYPE = np.dtype([(n, "<u8") for n in ("aligned_a", "aligned_b", "edits")] +
                          [(n, "<u4") for n in ("segments", "aligned", "backward", "too_long", "offband", "invalid", "overband", "reserved")])
# nts_edit_op: what Context.edit_script returns, one per edit
OP_DTYPE = np.dtype([("seg", "<u4"), ("p", "<u4"), ("q", "<u4"), ("op", "u1"), ("base_a", "u1"), ("base_b", "u1"), ("pad", "u1")])
OP_SUB, OP_DEL, OP_INS = 1, 2, 3
SEG_CANDIDATE, SEG_BACKWARD, SEG_LONG, SEG_OFFBAND = 0, 1, 2, 3
EDIT_NOT_CANDIDATE, EDIT_PASSED, EDIT_OVERBAND, EDIT_INVALID = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC
NO_MATE = 0xFFFFFFFF
# nts_extend_task / nts_extend_result: what Context.edit_extend takes and returns, one per task
TASK_DTYPE = np.dtype([("pos_a", "<u8"), ("pos_b", "<u8"), ("rec_a", "<u4"), ("rec_b", "<u4"), ("n", "<u4"), ("m", "<u4"), ("flags", "<u4"), ("pad", "<u4")])
EXTEND_DTYPE = np.dtype([(n, "<u4") for n in ("ext_a", "ext_b", "edits", "valid_a", "valid_b")])
EXTEND_A_BACKWARDS, EXTEND_B_BACKWARDS, EXTEND_B_COMPLEMENT = 1, 2, 4
# nts_cig_piece / nts_cig_chain: what Context.cigar_build takes and returns; a CIGAR entry is len << 4 | code
PIECE_DTYPE = np.dtype([(n, "<u4") for n in ("chain", "n", "m", "flags")])
CHAIN_DTYPE = np.dtype([(n, "<u8") for n in ("first", "n_cig", "eq", "x", "ins", "del", "len_a", "len_b")])
CIG_REVERSED = 1
CIG_INS, CIG_DEL, CIG_EQ, CIG_X = 1, 2, 7, 8
# nts_cig_span: where Context.cigar_text finds a chain's bases -- record and start in the target (a, forwards) and the query (b; with
# CIG_B_BACKWARDS pos_b is its first base as read: backwards and complemented)
CIG_SPAN_DTYPE = np.dtype([("pos_a", "<u8"), ("pos_b", "<u8"), ("rec_a", "<u4"), ("rec_b", "<u4"), ("flags", "<u4"), ("pad", "<u4")])
CIG_B_BACKWARDS = 1
# nts_cig_pad_at: what Context.cigar_pad takes per chain; CIG_PAD: the code of the entries it adds (BAM's P)
CIG_PAD_AT_DTYPE = np.dtype([("group", "<u4"), ("reserved", "<u4"), ("t0", "<u8")])
CIG_PAD = 6
# nts_cig_depth_seg: what Context.cigar_depth returns, one per segment of constant (aligned, match, gap)
CIG_DEPTH_SEG_DTYPE = np.dtype([("start", "<u8"), ("end", "<u8"), ("group", "<u4"), ("aligned", "<u4"), ("match", "<u4"), ("gap", "<u4")])
# nts_cig_allele: what Context.cigar_alleles returns, one per allele of a group (kind: 1 SNV, 2 DEL, 3 INS)
CIG_ALLELE_DTYPE = np.dtype([("pos", "<u8"), ("len", "<u8"), ("ref_off", "<u8"), ("alt_off", "<u8"), ("carrier_first", "<u8"), ("group", "<u4"),
                             ("kind", "<u4"), ("n_carriers", "<u4"), ("reserved", "<u4")])
# nts_cig_profile_col: what Context.cigar_profile returns, one per variable column of a group (sub: CIG_PROFILE_REF for a reference base,
# else the column inside the slot in front of base pos; n: A C G T N; ref, call: a letter or `-`)
CIG_PROFILE_COL_DTYPE = np.dtype([("pos", "<u8"), ("group", "<u4"), ("sub", "<u4"), ("aligned", "<u4"), ("match", "<u4"), ("gap", "<u4"),
                                  ("n", "<u4", (5,)), ("ref", "u1"), ("call", "u1"), ("reserved", "u1", (6,))])
CIG_PROFILE_REF = 0xFFFFFFFF
# nts_lift_query / nts_lift_hit: what Context.cigar_lift takes and returns, one per query
LIFT_QUERY_DTYPE = np.dtype([("chain", "<u4"), ("side", "<u4"), ("pos", "<u8")])
LIFT_HIT_DTYPE = np.dtype([("pos", "<u8"), ("entry", "<u8"), ("off", "<u8"), ("code", "<u4"), ("reserved", "<u4")])
# nts_lift_range / nts_lift_stats: what Context.cigar_lift_stats takes and returns, one per range
LIFT_RANGE_DTYPE = np.dtype([("chain", "<u4"), ("side", "<u4"), ("lo", "<u8"), ("hi", "<u8")])
LIFT_STATS_DTYPE = np.dtype([(n, "<u8") for n in ("oth_lo", "oth_hi", "eq", "x", "src_gap", "oth_gap")] +
                            [("src_gaps", "<u4"), ("oth_gaps", "<u4"), ("reserved", "<u8")])
# nts_lift_link / nts_pair_range / nts_pair_stats: what Context.cigar_lift_pairs takes (one per linked chain, one per range) and returns
LIFT_LINK_DTYPE = np.dtype([("chain", "<u4"), ("reserved", "<u4"), ("a0", "<u8"), ("b0", "<u8")])
PAIR_RANGE_DTYPE = np.dtype([("pair", "<u4"), ("side", "<u4"), ("lo", "<u8"), ("hi", "<u8")])
PAIR_STATS_DTYPE = np.dtype([(n, "<u8") for n in ("src_lo", "src_hi", "oth_lo", "oth_hi", "eq", "x", "src_gap", "oth_gap", "src_open", "oth_open")] +
                            [(n, "<u4") for n in ("src_gaps", "oth_gaps", "link_lo", "link_hi", "n_links", "reserved")] + [("reserved2", "<u8", (3,))])

# nts_chain_block / nts_chain_pair: what Context.cigar_chain_blocks returns, one per block of a liftover chain and one per pair
CHAIN_BLOCK_DTYPE = np.dtype([(n, "<u8") for n in ("size", "dt", "dq")])
CHAIN_PAIR_DTYPE = np.dtype([(n, "<u8") for n in ("a0", "a1", "b0", "b1", "eq", "x", "first_block")] + [("n_blocks", "<u4"), ("reserved", "<u4")])


class Context:
    """One per GPU (owns a HIP stream)."""

    def __init__(self, device=0, variant=None):
        "variant: None = the product build of the library; 'experiments' = the build with the experiment switches (tests, measurements)"
        self.lib = _lib.load(variant)
        self.variant = variant                 # (contexts that share device memory come from ONE build: each build has its own allocation cache)
        h = c_vp()
        rc = self.lib.nts_init(int(device), ctypes.byref(h))
        if rc != 0:
            raise NtsError(f"nts_init({device}) failed: {self.lib.nts_last_error(None).decode()} "
                           "(a real MI355X is required; there is no CPU fallback)")
        self.h = h
        self.device = int(device)

    def check(self, rc, what=""):
        if rc != 0:
            raise NtsError(f"{what}: {self.lib.nts_last_error(self.h).decode()} (code {rc})")

    def sync(self):
        self.check(self.lib.nts_sync(self.h), "nts_sync")

    def profile(self, enable=True):
        "True/1: time every kernel group; 2: only the dominant kernels (cheaper for short calls); False/0: off"
        level = int(enable) if not isinstance(enable, bool) else (1 if enable else 0)
        self.check(self.lib.nts_profile(self.h, level), "nts_profile")

    def minhash_intervals_stats(self):
        "(sweeps of the slowest chunk, chunks, sweeps in all) of the last Genome.minhash_intervals on this context"
        p, c, t = _lib.u32(), _lib.u32(), u64()
        self.check(self.lib.nts_minhash_intervals_stats(self.h, ctypes.byref(p), ctypes.byref(c), ctypes.byref(t)), "nts_minhash_intervals_stats")
        return p.value, c.value, t.value

    def minhash_pairs(self, sketches, counts, pair_a, pair_b):
        """(shared, size) of the Mash distance for pairs of bottom-s sketches (nts_minhash_pairs): sketches [n, s] uint64 with
        counts[i] hashes used in row i; pair p compares rows pair_a[p] and pair_b[p].  Two uint32 arrays."""
        sk = np.ascontiguousarray(sketches, dtype=np.uint64)
        cnt = np.ascontiguousarray(counts, dtype=np.uint32)
        a = np.ascontiguousarray(pair_a, dtype=np.uint64)
        b = np.ascontiguousarray(pair_b, dtype=np.uint64)
        if sk.ndim != 2 or cnt.size != sk.shape[0] or a.size != b.size:
            raise ValueError("minhash_pairs: sketches [n, s], one count per row, pair lists of one length")
        shared = np.zeros(a.size, dtype=np.uint32)
        size = np.zeros(a.size, dtype=np.uint32)
        self.check(self.lib.nts_minhash_pairs(self.h, sk.shape[1], sk.ctypes.data, cnt.ctypes.data, sk.shape[0], a.ctypes.data, b.ctypes.data,
                                              a.size, shared.ctypes.data, size.ctypes.data), "nts_minhash_pairs")
        return shared, size

    def iv_links(self, lists, min_anchors):
        """the sampled k-mers of several lists of intervals joined by hash (nts_iv_links).  lists: one SAMPLE_DTYPE array per genome, as
        Genome.bf_sample_intervals returns them (iv = the interval's index within that list).  Returns a LINK_DTYPE array sorted by
        (list_a, iv_a, list_b, iv_b): every pair of intervals of different lists with at least min_anchors hashes in common among
        those no list has twice."""
        arrs = [np.ascontiguousarray(a, dtype=SAMPLE_DTYPE) for a in lists]
        assert SAMPLE_DTYPE.itemsize == ctypes.sizeof(_lib.Sample) and LINK_DTYPE.itemsize == ctypes.sizeof(_lib.IvLink)
        ptrs = (c_vp * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
        counts = np.array([a.size for a in arrs], dtype=np.uint64)
        p, n = c_vp(), u64()
        self.check(self.lib.nts_iv_links(self.h, len(arrs), ptrs, counts.ctypes.data_as(_lib.c_u64p), int(min_anchors), ctypes.byref(p),
                                         ctypes.byref(n)), "nts_iv_links")
        out = np.empty(n.value, dtype=LINK_DTYPE)
        if n.value:
            ctypes.memmove(out.ctypes.data, p.value, out.nbytes)
        self.lib.nts_free(p)
        return out

    def iv_sites(self, lists, target, step, min_hits):
        """the sampled k-mers of several lists of gaps joined by hash against one genome's occurrence records, multiplicity allowed on
        both sides, and grouped into sites (nts_iv_sites).  lists: one SAMPLE_DTYPE array per genome (iv = the gap's index within that
        list); target: a SAMPLE_DTYPE array with iv = record index and off = position, as Genome.hset_sample_intervals_capped
        returns it for one interval per record.  Returns a SITE_DTYPE array sorted by (list_q, iv_q, rec_t, first_t): per gap, every
        maximal run of its pairs within one record whose consecutive positions differ by at most `step`, with at least min_hits
        pairs."""
        arrs = [np.ascontiguousarray(a, dtype=SAMPLE_DTYPE) for a in lists]
        tgt = np.ascontiguousarray(target, dtype=SAMPLE_DTYPE)
        assert SAMPLE_DTYPE.itemsize == ctypes.sizeof(_lib.Sample) and SITE_DTYPE.itemsize == ctypes.sizeof(_lib.IvSite)
        ptrs = (c_vp * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
        counts = np.array([a.size for a in arrs], dtype=np.uint64)
        p, n = c_vp(), u64()
        self.check(self.lib.nts_iv_sites(self.h, len(arrs), ptrs, counts.ctypes.data_as(_lib.c_u64p), tgt.ctypes.data if tgt.size else None, tgt.size,
                                         int(step), int(min_hits), ctypes.byref(p), ctypes.byref(n)), "nts_iv_sites")
        out = np.empty(n.value, dtype=SITE_DTYPE)
        if n.value:
            ctypes.memmove(out.ctypes.data, p.value, out.nbytes)
        self.lib.nts_free(p)
        return out

    def iv_periods(self, records, n_iv):
        """per interval the dominant lag between the recurrences of a hash among its sampled records (nts_iv_periods).  records: ONE
        SAMPLE_DTYPE array as a sampler returns it (Genome.sample_intervals: iv does not decrease, off rises strictly within an iv);
        n_iv: the intervals of that call.  Returns a PERIOD_DTYPE array of n_iv entries: recurring = the records that repeat the hash of
        an earlier record of their interval, period = the distance to that record held by the most of them (the smallest on a tie),
        period_hits = how many hold it, first_off / last_off = the smallest off - period / the largest off among those; zeros where
        nothing recurs.  Exact and deterministic."""
        rec = np.ascontiguousarray(records, dtype=SAMPLE_DTYPE)
        assert SAMPLE_DTYPE.itemsize == ctypes.sizeof(_lib.Sample) and PERIOD_DTYPE.itemsize == ctypes.sizeof(_lib.IvPeriod)
        out = np.zeros(int(n_iv), dtype=PERIOD_DTYPE)
        self.check(self.lib.nts_iv_periods(self.h, rec.ctypes.data if rec.size else None, rec.size, int(n_iv), out.ctypes.data if out.size else None),
                   "nts_iv_periods")
        return out

    def _take(self, p, n, dtype):
        "n elements of the library's array p as a numpy array of its own; p is released"
        out = np.empty(int(n), dtype=dtype)
        if out.size:
            ctypes.memmove(out.ctypes.data, p.value, out.nbytes)
        self.lib.nts_free(p)
        return out

    def iv_period_hashes(self, records, n_iv, period):
        """per interval the distinct hashes that carry its period (nts_iv_period_hashes).  records: ONE SAMPLE_DTYPE array as a sampler
        returns it (as for iv_periods); period: one value per interval, 0 = skip it.  Returns a SAMPLE_DTYPE array sorted by (iv, h0):
        one record per distinct (iv, h0) that has at least one record whose lag equals period[iv], off = how many such records there
        are.  Exact and deterministic."""
        rec = np.ascontiguousarray(records, dtype=SAMPLE_DTYPE)
        per = np.ascontiguousarray(period, dtype=np.uint32)
        if per.shape != (int(n_iv),):
            raise ValueError("iv_period_hashes: one period per interval")
        p, m = c_vp(), u64()
        self.check(self.lib.nts_iv_period_hashes(self.h, rec.ctypes.data if rec.size else None, rec.size, int(n_iv), per.ctypes.data if per.size else None,
                                                 ctypes.byref(p), ctypes.byref(m)), "nts_iv_period_hashes")
        return self._take(p, m.value, SAMPLE_DTYPE)

    def iv_families(self, pairs, n_arrays):
        """the arrays that share a hash joined into families (nts_iv_families).  pairs: a SAMPLE_DTYPE array of (h0, iv = the array's
        index; off is ignored, duplicates are allowed).  Returns (family, hashes, hash_family): family[a] = the smallest array index of
        a's component (a itself without a pair), hashes = the distinct h0 ascending, hash_family[j] = the component of hashes[j]."""
        rec = np.ascontiguousarray(pairs, dtype=SAMPLE_DTYPE)
        family = np.zeros(int(n_arrays), dtype=np.uint32)
        ph, pf, m = c_vp(), c_vp(), u64()
        self.check(self.lib.nts_iv_families(self.h, rec.ctypes.data if rec.size else None, rec.size, int(n_arrays), family.ctypes.data if family.size else None,
                                            ctypes.byref(ph), ctypes.byref(pf), ctypes.byref(m)), "nts_iv_families")
        return family, self._take(ph, m.value, np.uint64), self._take(pf, m.value, np.uint32)

    def iv_family_sites(self, occurrences, hashes, hash_family, step, min_hits):
        """where ONE genome holds each family's hashes close together (nts_iv_family_sites).  occurrences: the records of
        Genome.hset_sample_intervals over whole records (iv = record, off = position); hashes: ascending strictly, hash_family: the
        family of each.  Returns a FSITE_DTYPE array sorted by (family, rec, first): per family the maximal runs within one record
        whose consecutive positions differ by at most `step`, kept with at least min_hits occurrences; first / last = the first and
        the last position.  Exact and deterministic."""
        occ = np.ascontiguousarray(occurrences, dtype=SAMPLE_DTYPE)
        hs = np.ascontiguousarray(hashes, dtype=np.uint64)
        hf = np.ascontiguousarray(hash_family, dtype=np.uint32)
        if hs.ndim != 1 or hf.shape != hs.shape:
            raise ValueError("iv_family_sites: one family per hash")
        assert FSITE_DTYPE.itemsize == ctypes.sizeof(_lib.IvFsite)
        p, m = c_vp(), u64()
        self.check(self.lib.nts_iv_family_sites(self.h, occ.ctypes.data if occ.size else None, occ.size, hs.ctypes.data if hs.size else None,
                                                hf.ctypes.data if hf.size else None, hs.size, int(step), int(min_hits), ctypes.byref(p), ctypes.byref(m)),
                   "nts_iv_family_sites")
        return self._take(p, m.value, FSITE_DTYPE)

    def iv_anchor_segments(self, records_a, records_b, mate, len_b, flip, k, band, max_len):
        """the anchors of pairs of intervals of two genomes and the segments between consecutive anchors (nts_iv_anchor_segments).
        records_a / records_b: ONE SAMPLE_DTYPE array per genome as Genome.sample_intervals returns it; mate[i] = the interval of B
        paired with interval i of A (NO_MATE: none), len_b[i] = its clipped length, flip[i] = 1 when the strands differ.  An anchor
        is a hash either genome has exactly once, in two intervals that are mates.  Returns (segments, anchors_per_iv): a
        SEGMENT_DTYPE array in (iv_a, x) order with kind SEG_CANDIDATE / SEG_BACKWARD / SEG_LONG / SEG_OFFBAND, and the anchors of each
        interval of A [n_iv_a] uint32.  Exact and deterministic."""
        ra = np.ascontiguousarray(records_a, dtype=SAMPLE_DTYPE)
        rb = np.ascontiguousarray(records_b, dtype=SAMPLE_DTYPE)
        mt = np.ascontiguousarray(mate, dtype=np.uint32)
        lb = np.ascontiguousarray(len_b, dtype=np.uint32)
        fl = np.ascontiguousarray(flip, dtype=np.uint8)
        if mt.ndim != 1 or lb.shape != mt.shape or fl.shape != mt.shape:
            raise ValueError("iv_anchor_segments: one mate, length and flip per interval of A")
        assert SEGMENT_DTYPE.itemsize == ctypes.sizeof(_lib.IvSegment)
        per_iv = np.zeros(mt.size, dtype=np.uint32)
        p, m = c_vp(), u64()
        self.check(self.lib.nts_iv_anchor_segments(self.h, ra.ctypes.data if ra.size else None, ra.size, rb.ctypes.data if rb.size else None, rb.size,
                                                   mt.ctypes.data if mt.size else None, mt.size, lb.ctypes.data if mt.size else None,
                                                   fl.ctypes.data if mt.size else None, int(k), int(band), int(max_len), ctypes.byref(p), ctypes.byref(m),
                                                   per_iv.ctypes.data if mt.size else None), "nts_iv_anchor_segments")
        return self._take(p, m.value, SEGMENT_DTYPE), per_iv

    def edit_segments(self, genome_a, genome_b, intervals_a, intervals_b, segments, flip, band, with_distances=False):
        """the exact edit distance of every candidate segment and the sums per interval (nts_edit_segments).  intervals_a /
        intervals_b: (rec, start, end) rows, row i of intervals_b being the MATE of A's interval i; segments: a SEGMENT_DTYPE array in
        iv_a order; flip[i] = 1: B's interval is read as its reverse complement.  Returns an IDENTITY_DTYPE array, one entry per
        interval of A -- and with with_distances the per-segment results [n] uint32: the distance, or EDIT_PASSED / EDIT_INVALID /
        EDIT_OVERBAND / EDIT_NOT_CANDIDATE.  Exact and deterministic."""
        iva = Genome._interval_array(intervals_a)
        ivb = Genome._interval_array(intervals_b)
        seg = np.ascontiguousarray(segments, dtype=SEGMENT_DTYPE)
        fl = np.ascontiguousarray(flip, dtype=np.uint8)
        if ivb.size != iva.size or fl.shape != (iva.size,):
            raise ValueError("edit_segments: one interval of B and one flip per interval of A")
        assert IDENTITY_DTYPE.itemsize == ctypes.sizeof(_lib.IvIdentity)
        out = np.zeros(iva.size, dtype=IDENTITY_DTYPE)
        dist = np.zeros(seg.size, dtype=np.uint32) if with_distances else None
        self.check(self.lib.nts_edit_segments(self.h, genome_a.h, genome_b.h, ctypes.cast(iva.ctypes.data, ctypes.POINTER(Interval)),
                                              ctypes.cast(ivb.ctypes.data, ctypes.POINTER(Interval)), seg.ctypes.data if seg.size else None, seg.size,
                                              iva.size, fl.ctypes.data if fl.size else None, int(band), out.ctypes.data if out.size else None,
                                              dist.ctypes.data if with_distances and dist.size else None), "nts_edit_segments")
        return (out, dist) if with_distances else out

    def edit_script(self, genome_a, genome_b, intervals_a, intervals_b, segments, flip, band, dist):
        """the edits behind every segment's distance (nts_edit_script): the arguments of edit_segments and the per-segment results it
        returns with with_distances.  Returns (ops, first): an OP_DTYPE array with the canonical script of every segment that has a
        distance, one behind the other in segment order and each in path order, and first [n + 1] uint64 -- segment i's ops are
        ops[first[i]:first[i + 1]].  op is OP_SUB / OP_DEL / OP_INS at offset p of string A and q of the oriented string B; base_a /
        base_b are the codes of A[p] and of the oriented B[q], 0xFF where the op has none.  A dist that is not the segments' own is
        refused.  Exact and deterministic."""
        iva = Genome._interval_array(intervals_a)
        ivb = Genome._interval_array(intervals_b)
        seg = np.ascontiguousarray(segments, dtype=SEGMENT_DTYPE)
        fl = np.ascontiguousarray(flip, dtype=np.uint8)
        ds = np.ascontiguousarray(dist, dtype=np.uint32)
        if ivb.size != iva.size or fl.shape != (iva.size,):
            raise ValueError("edit_script: one interval of B and one flip per interval of A")
        if ds.shape != (seg.size,):
            raise ValueError("edit_script: one dist per segment")
        assert OP_DTYPE.itemsize == ctypes.sizeof(_lib.EditOp)
        first = np.zeros(seg.size + 1, dtype=np.uint64)
        p, m = c_vp(), u64()
        self.check(self.lib.nts_edit_script(self.h, genome_a.h, genome_b.h, ctypes.cast(iva.ctypes.data, ctypes.POINTER(Interval)),
                                            ctypes.cast(ivb.ctypes.data, ctypes.POINTER(Interval)), seg.ctypes.data if seg.size else None, seg.size,
                                            iva.size, fl.ctypes.data if fl.size else None, int(band), ds.ctypes.data if ds.size else None,
                                            ctypes.byref(p), ctypes.byref(m), first.ctypes.data), "nts_edit_script")
        return self._take(p, m.value, OP_DTYPE), first

    def edit_wide(self, genome_a, genome_b, intervals_a, intervals_b, segments, flip, band, max_edits, dist):
        """the stretches the band leaves out (nts_edit_wide): the arguments of edit_segments, max_edits = E in 2 band + 1 .. 1023 and the
        per-segment results edit_segments returns with with_distances.  The unrestricted edit distance of every offband segment with
        |dy - dx| <= E and of every candidate that came back EDIT_OVERBAND: the distance where it is at most E, else EDIT_OVERBAND, or
        EDIT_INVALID; every other entry as it was.  Returns (an IDENTITY_DTYPE array over the final results, one entry per interval of
        A; the final per-segment results [n] uint32).  A dist that contradicts a segment's kind is refused.  Exact and deterministic."""
        iva = Genome._interval_array(intervals_a)
        ivb = Genome._interval_array(intervals_b)
        seg = np.ascontiguousarray(segments, dtype=SEGMENT_DTYPE)
        fl = np.ascontiguousarray(flip, dtype=np.uint8)
        ds = np.ascontiguousarray(dist, dtype=np.uint32)
        if ivb.size != iva.size or fl.shape != (iva.size,):
            raise ValueError("edit_wide: one interval of B and one flip per interval of A")
        if ds.shape != (seg.size,):
            raise ValueError("edit_wide: one dist per segment")
        assert IDENTITY_DTYPE.itemsize == ctypes.sizeof(_lib.IvIdentity)
        out = np.zeros(iva.size, dtype=IDENTITY_DTYPE)
        final = np.zeros(seg.size, dtype=np.uint32)
        self.check(self.lib.nts_edit_wide(self.h, genome_a.h, genome_b.h, ctypes.cast(iva.ctypes.data, ctypes.POINTER(Interval)),
                                          ctypes.cast(ivb.ctypes.data, ctypes.POINTER(Interval)), seg.ctypes.data if seg.size else None, seg.size,
                                          iva.size, fl.ctypes.data if fl.size else None, int(band), int(max_edits), ds.ctypes.data if ds.size else None,
                                          out.ctypes.data if out.size else None, final.ctypes.data if final.size else None), "nts_edit_wide")
        return out, final

    def edit_wide_script(self, genome_a, genome_b, intervals_a, intervals_b, segments, flip, band, max_edits, dist, table_budget=0):
        """the edits of the stretches beyond the band (nts_edit_wide_script): the arguments of edit_wide and the final per-segment
        results it returns.  The script set: every segment with a distance that edit_script does not take -- kind offband, or a
        candidate with D + |dy - dx| > 2 band + 1.  Returns (ops, first) as edit_script does: the canonical script of every member in
        an OP_DTYPE array, member i's ops at ops[first[i]:first[i + 1]]; every other segment adds nothing.  table_budget: the bytes the
        members' furthest-reaching tables may take at once (0 = 1 GiB; at least 4 (max_edits + 1)^2); the result does not depend on it.
        A dist that is not the segments' own is refused.  Exact and deterministic."""
        iva = Genome._interval_array(intervals_a)
        ivb = Genome._interval_array(intervals_b)
        seg = np.ascontiguousarray(segments, dtype=SEGMENT_DTYPE)
        fl = np.ascontiguousarray(flip, dtype=np.uint8)
        ds = np.ascontiguousarray(dist, dtype=np.uint32)
        if ivb.size != iva.size or fl.shape != (iva.size,):
            raise ValueError("edit_wide_script: one interval of B and one flip per interval of A")
        if ds.shape != (seg.size,):
            raise ValueError("edit_wide_script: one dist per segment")
        if int(table_budget) < 0:
            raise ValueError("edit_wide_script: table_budget is a number of bytes, 0 for the default")
        assert OP_DTYPE.itemsize == ctypes.sizeof(_lib.EditOp)
        first = np.zeros(seg.size + 1, dtype=np.uint64)
        p, m = c_vp(), u64()
        self.check(self.lib.nts_edit_wide_script(self.h, genome_a.h, genome_b.h, ctypes.cast(iva.ctypes.data, ctypes.POINTER(Interval)),
                                                 ctypes.cast(ivb.ctypes.data, ctypes.POINTER(Interval)), seg.ctypes.data if seg.size else None, seg.size,
                                                 iva.size, fl.ctypes.data if fl.size else None, int(band), int(max_edits),
                                                 ds.ctypes.data if ds.size else None, int(table_budget), ctypes.byref(p), ctypes.byref(m),
                                                 first.ctypes.data), "nts_edit_wide_script")
        return self._take(p, m.value, OP_DTYPE), first

    def edit_wide_script_last_plan(self):
        "dict(members, table_bytes, batches) of the last edit_wide_script on this context (nts_edit_wide_script_last_plan)"
        a, b, c = u64(), u64(), u64()
        self.check(self.lib.nts_edit_wide_script_last_plan(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "nts_edit_wide_script_last_plan")
        return {"members": a.value, "table_bytes": b.value, "batches": c.value}

    def edit_extend(self, genome_a, genome_b, tasks, penalty, max_edits, out=None):
        """how far two strings stay alignable from a common start (nts_edit_extend).  tasks: a TASK_DTYPE array -- n bases of record
        rec_a of genome_a from pos_a and m bases of record rec_b of genome_b from pos_b, flags: EXTEND_A_BACKWARDS, EXTEND_B_BACKWARDS,
        EXTEND_B_COMPLEMENT.  Both strings are cut before their first base that is not A, C, G or T; among the cells of the unrestricted
        edit table with at most max_edits = E (1..1023) edits the one with the largest i + j - penalty * edits (penalty 3..255), ties to
        the fewest edits, then to the least j - i.  Returns an EXTEND_DTYPE array (ext_a, ext_b, edits, valid_a, valid_b), one entry per
        task -- `out` itself when given, which a refused call leaves untouched.  Exact and deterministic."""
        tk = np.ascontiguousarray(tasks, dtype=TASK_DTYPE)
        if tk.ndim != 1:
            raise ValueError("edit_extend: a list of tasks")
        assert TASK_DTYPE.itemsize == ctypes.sizeof(_lib.ExtendTask) and EXTEND_DTYPE.itemsize == ctypes.sizeof(_lib.ExtendResult)
        if out is None:
            out = np.zeros(tk.size, dtype=EXTEND_DTYPE)
        if out.dtype != EXTEND_DTYPE or out.shape != (tk.size,) or not out.flags.c_contiguous:
            raise ValueError("edit_extend: out is a contiguous EXTEND_DTYPE array, one entry per task")
        self.check(self.lib.nts_edit_extend(self.h, genome_a.h, genome_b.h, tk.ctypes.data if tk.size else None, tk.size, int(penalty), int(max_edits),
                                            out.ctypes.data if out.size else None), "nts_edit_extend")
        return out

    def edit_extend_script(self, genome_a, genome_b, tasks, results, table_budget=0):
        """the edits of the extended flanks (nts_edit_extend_script): the tasks of edit_extend and the results it returned for them.  For
        task t the canonical script (as edit_script defines it) of the first ext_a bases of its string A and the first ext_b bases of
        its string B, both as edit_extend reads them.  Returns (ops, first): an OP_DTYPE array with task t's `edits` ops at
        ops[first[t]:first[t + 1]], seg = t, p and q offsets in the strings as read, base_b complemented as read.  table_budget: the
        bytes the tasks' furthest-reaching tables may take at once (0 = 1 GiB; at least 4 (Dmax + 1)^2 for the largest `edits`); the
        result does not depend on it.  Results that are not the tasks' own are refused.  Exact and deterministic."""
        tk = np.ascontiguousarray(tasks, dtype=TASK_DTYPE)
        rs = np.ascontiguousarray(results, dtype=EXTEND_DTYPE)
        if tk.ndim != 1 or rs.shape != tk.shape:
            raise ValueError("edit_extend_script: a list of tasks and one result per task")
        if int(table_budget) < 0:
            raise ValueError("edit_extend_script: table_budget is a number of bytes, 0 for the default")
        assert TASK_DTYPE.itemsize == ctypes.sizeof(_lib.ExtendTask) and EXTEND_DTYPE.itemsize == ctypes.sizeof(_lib.ExtendResult)
        assert OP_DTYPE.itemsize == ctypes.sizeof(_lib.EditOp)
        first = np.zeros(tk.size + 1, dtype=np.uint64)
        p, m = c_vp(), u64()
        self.check(self.lib.nts_edit_extend_script(self.h, genome_a.h, genome_b.h, tk.ctypes.data if tk.size else None, tk.size,
                                                   rs.ctypes.data if rs.size else None, int(table_budget), ctypes.byref(p), ctypes.byref(m),
                                                   first.ctypes.data), "nts_edit_extend_script")
        return self._take(p, m.value, OP_DTYPE), first

    def edit_extend_script_last_plan(self):
        "dict(members, table_bytes, batches) of the last edit_extend_script on this context (nts_edit_extend_script_last_plan)"
        a, b, c = u64(), u64(), u64()
        self.check(self.lib.nts_edit_extend_script_last_plan(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "nts_edit_extend_script_last_plan")
        return {"members": a.value, "table_bytes": b.value, "batches": c.value}

    def cigar_build(self, pieces, ops, first, n_chains):
        """one CIGAR per chain of aligned pieces (nts_cigar_build).  pieces: a PIECE_DTYPE array in chain order -- two strings of n and
        m bases, flags CIG_REVERSED for a piece whose columns are taken backwards; ops: an OP_DTYPE array, the scripts of all pieces one
        behind the other with seg = the piece's index and p, q local to the piece; first [len(pieces) + 1]: piece t's ops are
        ops[first[t]:first[t + 1]].  Returns (cigar, chains): cigar [E] uint64, entries len << 4 | code (CIG_INS 1, CIG_DEL 2, CIG_EQ 7,
        CIG_X 8) of all chains one behind the other, runs of one kind merged across pieces and never across chains; chains a
        CHAIN_DTYPE array of n_chains entries -- chain c's entries are cigar[first:first + n_cig], eq / x / ins / del its columns of
        each kind, len_a and len_b the bases of either side.  Ops that are no script of their piece's lengths are refused.  No genome
        is read.  Exact and deterministic."""
        pc = np.ascontiguousarray(pieces, dtype=PIECE_DTYPE)
        op = np.ascontiguousarray(ops, dtype=OP_DTYPE)
        ft = np.ascontiguousarray(first, dtype=np.uint64)
        if pc.ndim != 1 or op.ndim != 1 or ft.shape != (pc.size + 1,):
            raise ValueError("cigar_build: a list of pieces, a list of ops and one first entry per piece plus one")
        if int(ft[-1]) != op.size:
            raise ValueError("cigar_build: first ends at the number of ops")
        if int(n_chains) < 0:
            raise ValueError("cigar_build: n_chains is a count")
        assert PIECE_DTYPE.itemsize == ctypes.sizeof(_lib.CigPiece) and CHAIN_DTYPE.itemsize == ctypes.sizeof(_lib.CigChain)
        assert OP_DTYPE.itemsize == ctypes.sizeof(_lib.EditOp)
        chains = np.zeros(int(n_chains), dtype=CHAIN_DTYPE)
        p, m = c_vp(), u64()
        self.check(self.lib.nts_cigar_build(self.h, pc.ctypes.data if pc.size else None, pc.size, int(n_chains), op.ctypes.data if op.size else None,
                                            ft.ctypes.data, ctypes.byref(p), ctypes.byref(m), chains.ctypes.data if chains.size else None),
                   "nts_cigar_build")
        return self._take(p, m.value, np.dtype("<u8")), chains

    def cigar_text(self, cigar, chains, spans=None, genome_a=None, genome_b=None):
        """the cg:Z: and cs:Z: texts of the chains' CIGARs (nts_cigar_text).  cigar [E] uint64 and chains, a CHAIN_DTYPE array: what
        cigar_build returns (entries need not be maximal runs; the chains tile the entries).  Without spans: returns (cg, cg_first) --
        cg a uint8 array, chain c's text is cg[cg_first[c]:cg_first[c + 1]], cg_first [len(chains) + 1] uint64 -- and no genome is
        read.  spans: a CIG_SPAN_DTYPE array, one per chain -- its len_a target bases are record rec_a of genome_a from pos_a on,
        forwards; its len_b query bases record rec_b of genome_b from pos_b on, or with CIG_B_BACKWARDS from pos_b downwards and
        complemented; returns (cg, cg_first, cs, cs_first), cs the short form (:n, *tq, -bases, +bases; lower case, n for what is no
        base).  Chains that do not tile the entries, entries that are no CIGAR of the chains' lengths, spans outside their records and
        texts of 2^32 bytes or more are refused.  Exact and deterministic."""
        cg = np.ascontiguousarray(cigar, dtype=np.uint64)
        ch = np.ascontiguousarray(chains, dtype=CHAIN_DTYPE)
        if cg.ndim != 1 or ch.ndim != 1:
            raise ValueError("cigar_text: a list of entries and a list of chain records")
        if spans is None and (genome_a is not None or genome_b is not None):
            raise ValueError("cigar_text: genomes go with spans")
        assert CHAIN_DTYPE.itemsize == ctypes.sizeof(_lib.CigChain) and CIG_SPAN_DTYPE.itemsize == ctypes.sizeof(_lib.CigSpan)
        sp = None
        if spans is not None:
            sp = np.ascontiguousarray(spans, dtype=CIG_SPAN_DTYPE)
            if sp.shape != (ch.size,):
                raise ValueError("cigar_text: one span per chain")
            if genome_a is None or genome_b is None:
                raise ValueError("cigar_text: spans go with both genomes")
            if sp.size == 0:
                sp = np.zeros(1, dtype=CIG_SPAN_DTYPE)       # (a pointer that is not NULL: spans were given)
        firsts = np.zeros((2, ch.size + 1), dtype=np.uint64)
        p_cg, p_cs = c_vp(), c_vp()
        self.check(self.lib.nts_cigar_text(self.h, cg.ctypes.data if cg.size else None, cg.size, ch.ctypes.data if ch.size else None, ch.size,
                                           genome_a.h if sp is not None else None, genome_b.h if sp is not None else None,
                                           sp.ctypes.data if sp is not None else None, ctypes.byref(p_cg), firsts[0].ctypes.data,
                                           ctypes.byref(p_cs) if sp is not None else None, firsts[1].ctypes.data if sp is not None else None),
                   "nts_cigar_text")
        text = self._take(p_cg, int(firsts[0, -1]), np.dtype("u1"))
        if sp is None:
            return text, firsts[0].copy()
        return text, firsts[0].copy(), self._take(p_cs, int(firsts[1, -1]), np.dtype("u1")), firsts[1].copy()

    def cigar_pad(self, cigar, chains, at, n_groups=None):
        """the padded CIGARs of a reference-anchored multiple alignment (nts_cigar_pad).  cigar and chains as cigar_build returns them,
        the chains tiling the entries and every non-empty chain beginning and ending with an = or X entry; at: a CIG_PAD_AT_DTYPE
        array, one {group, t0} per chain -- the chains of a group are aligned to one reference record, chain c covering its bases
        [t0, t0 + len_a); groups nondecreasing and below n_groups (default: the last chain's group + 1).  Returns (padded, pad_first,
        site_first, site_pos, site_w), all uint64: chain c's entries with the entries of code CIG_PAD it needs are
        padded[pad_first[c]:pad_first[c + 1]]; group g's sites -- the slots in front of a reference base that hold an I entry of the
        group -- are site_pos[site_first[g]:site_first[g + 1]], ascending, their widths site_w.  Reads no genome.  Exact and
        deterministic."""
        cg = np.ascontiguousarray(cigar, dtype=np.uint64)
        ch = np.ascontiguousarray(chains, dtype=CHAIN_DTYPE)
        where = np.ascontiguousarray(at, dtype=CIG_PAD_AT_DTYPE)
        if cg.ndim != 1 or ch.ndim != 1 or where.shape != ch.shape:
            raise ValueError("cigar_pad: a list of entries, a list of chain records and one {group, t0} per chain")
        assert CHAIN_DTYPE.itemsize == ctypes.sizeof(_lib.CigChain) and CIG_PAD_AT_DTYPE.itemsize == ctypes.sizeof(_lib.CigPadAt)
        if n_groups is None:
            n_groups = int(where["group"][-1]) + 1 if where.size else 0
        pad_first = np.zeros(ch.size + 1, dtype=np.uint64)
        site_first = np.zeros(int(n_groups) + 1, dtype=np.uint64)
        p_out, p_pos, p_w = c_vp(), c_vp(), c_vp()
        self.check(self.lib.nts_cigar_pad(self.h, cg.ctypes.data if cg.size else None, cg.size, ch.ctypes.data if ch.size else None, ch.size,
                                          where.ctypes.data if where.size else None, int(n_groups), ctypes.byref(p_out), pad_first.ctypes.data,
                                          site_first.ctypes.data, ctypes.byref(p_pos), ctypes.byref(p_w)), "nts_cigar_pad")
        n_sites = int(site_first[-1])
        return (self._take(p_out, int(pad_first[-1]), np.dtype("<u8")), pad_first, site_first, self._take(p_pos, n_sites, np.dtype("<u8")),
                self._take(p_w, n_sites, np.dtype("<u8")))

    def cigar_depth(self, cigar, chains, at, n_groups=None):
        """per-base depth and identity over a reference-anchored group of chains (nts_cigar_depth).  cigar, chains, at and n_groups as
        for cigar_pad, but the chains need not be cores, the entries need not be maximal runs and chains of a group may overlap.
        Returns (segs, seg_first): a CIG_DEPTH_SEG_DTYPE array of the maximal runs [start, end) of reference bases of one group with
        aligned > 0 and one (aligned, match, gap) -- the chains covering a base, those with an = there, those with a D there --
        ascending by (group, start), and seg_first [n_groups + 1] uint64: group g's are segs[seg_first[g]:seg_first[g + 1]].  Reads no
        genome.  Exact and deterministic."""
        cg = np.ascontiguousarray(cigar, dtype=np.uint64)
        ch = np.ascontiguousarray(chains, dtype=CHAIN_DTYPE)
        where = np.ascontiguousarray(at, dtype=CIG_PAD_AT_DTYPE)
        if cg.ndim != 1 or ch.ndim != 1 or where.shape != ch.shape:
            raise ValueError("cigar_depth: a list of entries, a list of chain records and one {group, t0} per chain")
        assert CHAIN_DTYPE.itemsize == ctypes.sizeof(_lib.CigChain) and CIG_PAD_AT_DTYPE.itemsize == ctypes.sizeof(_lib.CigPadAt)
        assert CIG_DEPTH_SEG_DTYPE.itemsize == ctypes.sizeof(_lib.CigDepthSeg)
        if n_groups is None:
            n_groups = int(where["group"][-1]) + 1 if where.size else 0
        seg_first = np.zeros(int(n_groups) + 1, dtype=np.uint64)
        p_segs = c_vp()
        self.check(self.lib.nts_cigar_depth(self.h, cg.ctypes.data if cg.size else None, cg.size, ch.ctypes.data if ch.size else None, ch.size,
                                            where.ctypes.data if where.size else None, int(n_groups), ctypes.byref(p_segs), seg_first.ctypes.data),
                   "nts_cigar_depth")
        return self._take(p_segs, int(seg_first[-1]), CIG_DEPTH_SEG_DTYPE), seg_first

    def cigar_var_bases(self, cigar, chains, spans, genome_a, genome_b):
        """the bases at the variant columns of the chains' CIGARs (nts_cigar_var_bases).  Arguments, checks and refusals as cigar_rows'
        (entries of code CIG_PAD are refused).  Returns (ref, ref_first, alt, alt_first): ref holds, chain after chain, the bytes of
        cigar_rows' row A at the columns of the X and D entries, alt those of row B at the columns of the X and I entries -- upper case
        ACGT, N for what is no base --; chain c's are ref[ref_first[c]:ref_first[c + 1]] and alt[alt_first[c]:alt_first[c + 1]], the
        firsts [len(chains) + 1] uint64.  A buffer of 2^32 bytes or more is refused.  Exact and deterministic."""
        cg = np.ascontiguousarray(cigar, dtype=np.uint64)
        ch = np.ascontiguousarray(chains, dtype=CHAIN_DTYPE)
        if cg.ndim != 1 or ch.ndim != 1:
            raise ValueError("cigar_var_bases: a list of entries and a list of chain records")
        assert CHAIN_DTYPE.itemsize == ctypes.sizeof(_lib.CigChain) and CIG_SPAN_DTYPE.itemsize == ctypes.sizeof(_lib.CigSpan)
        sp = None
        if spans is not None:
            sp = np.ascontiguousarray(spans, dtype=CIG_SPAN_DTYPE)
            if sp.shape != (ch.size,):
                raise ValueError("cigar_var_bases: one span per chain")
            if sp.size == 0:
                sp = np.zeros(1, dtype=CIG_SPAN_DTYPE)       # (a pointer that is not NULL: spans were given)
        ref_first, alt_first = np.zeros(ch.size + 1, dtype=np.uint64), np.zeros(ch.size + 1, dtype=np.uint64)
        p_ref, p_alt = c_vp(), c_vp()
        self.check(self.lib.nts_cigar_var_bases(self.h, cg.ctypes.data if cg.size else None, cg.size, ch.ctypes.data if ch.size else None, ch.size,
                                                genome_a.h if genome_a is not None else None, genome_b.h if genome_b is not None else None,
                                                sp.ctypes.data if sp is not None else None, ctypes.byref(p_ref), ref_first.ctypes.data,
                                                ctypes.byref(p_alt), alt_first.ctypes.data), "nts_cigar_var_bases")
        return self._take(p_ref, int(ref_first[-1]), np.dtype("u1")), ref_first, self._take(p_alt, int(alt_first[-1]), np.dtype("u1")), alt_first

    def cigar_alleles(self, cigar, chains, at, alt, n_groups=None):
        """one allele table per reference-anchored group of chains (nts_cigar_alleles).  cigar, chains, at and n_groups as for cigar_pad
        (the chains are cores and tile the entries; chains of a group may overlap); alt: the alt bytes of cigar_var_bases over all
        chains in chain order, uint8.  Returns (alleles, allele_first, carriers): a CIG_ALLELE_DTYPE array -- an allele is the events
        (an X column: kind 1, a D entry: kind 2, an I entry: kind 3) of equal (group, pos, kind, len, alt bytes) -- ascending by (group,
        pos, kind, len or alt byte, smallest carrier), group g's being alleles[allele_first[g]:allele_first[g + 1]] (allele_first
        [n_groups + 1] uint64), and carriers, uint32: the chains that hold allele r are carriers[carrier_first:carrier_first +
        n_carriers], ascending; ref_off and alt_off: the bytes of its smallest carrier in cigar_var_bases' buffers.  Reads no genome.
        Exact and deterministic."""
        cg = np.ascontiguousarray(cigar, dtype=np.uint64)
        ch = np.ascontiguousarray(chains, dtype=CHAIN_DTYPE)
        where = np.ascontiguousarray(at, dtype=CIG_PAD_AT_DTYPE)
        bases = np.ascontiguousarray(alt, dtype=np.uint8)
        if cg.ndim != 1 or ch.ndim != 1 or where.shape != ch.shape or bases.ndim != 1:
            raise ValueError("cigar_alleles: a list of entries, a list of chain records, one {group, t0} per chain and a list of bytes")
        assert CHAIN_DTYPE.itemsize == ctypes.sizeof(_lib.CigChain) and CIG_PAD_AT_DTYPE.itemsize == ctypes.sizeof(_lib.CigPadAt)
        assert CIG_ALLELE_DTYPE.itemsize == ctypes.sizeof(_lib.CigAllele) == 56
        if n_groups is None:
            n_groups = int(where["group"][-1]) + 1 if where.size else 0
        allele_first = np.zeros(int(n_groups) + 1, dtype=np.uint64)
        p_alleles, p_carriers, n_carriers = c_vp(), c_vp(), ctypes.c_uint64(0)
        self.check(self.lib.nts_cigar_alleles(self.h, cg.ctypes.data if cg.size else None, cg.size, ch.ctypes.data if ch.size else None, ch.size,
                                              where.ctypes.data if where.size else None, int(n_groups), bases.ctypes.data if bases.size else None,
                                              bases.size, ctypes.byref(p_alleles), allele_first.ctypes.data, ctypes.byref(p_carriers),
                                              ctypes.byref(n_carriers)), "nts_cigar_alleles")
        return self._take(p_alleles, int(allele_first[-1]), CIG_ALLELE_DTYPE), allele_first, self._take(p_carriers, int(n_carriers.value), np.dtype("<u4"))

    def cigar_profile(self, cigar, chains, at, ref, alt, n_groups=None):
        """the variable columns of every reference-anchored group of chains, with their counts and plurality call (nts_cigar_profile).
        cigar, chains, at and n_groups as for cigar_alleles (the chains are cores and tile the entries; chains of a group may overlap);
        ref, alt: the bytes of cigar_var_bases over all chains in chain order, uint8.  Returns (cols, col_first): a
        CIG_PROFILE_COL_DTYPE array -- one record per reference base at which a covering chain has an X or a D (sub CIG_PROFILE_REF)
        and per column of every insertion slot (sub: the column; pos: the base the slot lies in front of) -- ascending by (group, pos,
        sub), the multi-MAF's column order; group g's are cols[col_first[g]:col_first[g + 1]] (col_first [n_groups + 1] uint64).
        aligned: the chains covering the column (t0 <= pos < t1), match / gap: those with an = / a D there, n: those holding A, C, G, T
        or another byte there; ref: the reference's byte (`-` in a slot); call: the symbol with the largest tally, the reference row
        counted in, ties to the reference's symbol, else to the first of A C G T N -.  Reads no genome.  Exact and deterministic."""
        cg = np.ascontiguousarray(cigar, dtype=np.uint64)
        ch = np.ascontiguousarray(chains, dtype=CHAIN_DTYPE)
        where = np.ascontiguousarray(at, dtype=CIG_PAD_AT_DTYPE)
        ref_b, alt_b = np.ascontiguousarray(ref, dtype=np.uint8), np.ascontiguousarray(alt, dtype=np.uint8)
        if cg.ndim != 1 or ch.ndim != 1 or where.shape != ch.shape or ref_b.ndim != 1 or alt_b.ndim != 1:
            raise ValueError("cigar_profile: a list of entries, a list of chain records, one {group, t0} per chain and two lists of bytes")
        assert CHAIN_DTYPE.itemsize == ctypes.sizeof(_lib.CigChain) and CIG_PAD_AT_DTYPE.itemsize == ctypes.sizeof(_lib.CigPadAt)
        assert CIG_PROFILE_COL_DTYPE.itemsize == ctypes.sizeof(_lib.CigProfileCol) == 56
        if n_groups is None:
            n_groups = int(where["group"][-1]) + 1 if where.size else 0
        col_first = np.zeros(int(n_groups) + 1, dtype=np.uint64)
        p_cols = c_vp()
        self.check(self.lib.nts_cigar_profile(self.h, cg.ctypes.data if cg.size else None, cg.size, ch.ctypes.data if ch.size else None, ch.size,
                                              where.ctypes.data if where.size else None, int(n_groups), ref_b.ctypes.data if ref_b.size else None,
                                              ref_b.size, alt_b.ctypes.data if alt_b.size else None, alt_b.size, ctypes.byref(p_cols),
                                              col_first.ctypes.data), "nts_cigar_profile")
        return self._take(p_cols, int(col_first[-1]), CIG_PROFILE_COL_DTYPE), col_first

    def cigar_rows(self, cigar, chains, spans, genome_a, genome_b, padded=False):
        """the aligned rows of the chains' CIGARs, the sequence lines of a MAF block (nts_cigar_rows).  cigar, chains, spans and the
        genomes as for cigar_text with spans; all are required.  Returns (row_a, row_b, row_first): two uint8 arrays of equal length
        and row_first [len(chains) + 1] uint64 -- chain c's rows are row_a[row_first[c]:row_first[c + 1]] and the same slice of
        row_b, one byte per alignment column: row_a the target base (`-` for I), row_b the query base as read (`-` for D), upper case
        ACGT and N for what is no base.  Refusals as cigar_text's; rows of 2^32 columns or more are refused.  Exact and
        deterministic.  padded=True (nts_cigar_rows_padded): entries of code CIG_PAD, as cigar_pad adds them, are accepted: a column
        that is `-` in both rows and consumes no base; without it such an entry is refused."""
        cg = np.ascontiguousarray(cigar, dtype=np.uint64)
        ch = np.ascontiguousarray(chains, dtype=CHAIN_DTYPE)
        if cg.ndim != 1 or ch.ndim != 1:
            raise ValueError("cigar_rows: a list of entries and a list of chain records")
        assert CHAIN_DTYPE.itemsize == ctypes.sizeof(_lib.CigChain) and CIG_SPAN_DTYPE.itemsize == ctypes.sizeof(_lib.CigSpan)
        sp = None
        if spans is not None:
            sp = np.ascontiguousarray(spans, dtype=CIG_SPAN_DTYPE)
            if sp.shape != (ch.size,):
                raise ValueError("cigar_rows: one span per chain")
            if sp.size == 0:
                sp = np.zeros(1, dtype=CIG_SPAN_DTYPE)       # (a pointer that is not NULL: spans were given)
        first = np.zeros(ch.size + 1, dtype=np.uint64)
        p_a, p_b = c_vp(), c_vp()
        call, name = (self.lib.nts_cigar_rows_padded, "nts_cigar_rows_padded") if padded else (self.lib.nts_cigar_rows, "nts_cigar_rows")
        self.check(call(self.h, cg.ctypes.data if cg.size else None, cg.size, ch.ctypes.data if ch.size else None, ch.size,
                        genome_a.h if genome_a is not None else None, genome_b.h if genome_b is not None else None,
                        sp.ctypes.data if sp is not None else None, ctypes.byref(p_a), ctypes.byref(p_b), first.ctypes.data), name)
        n = int(first[-1])
        return self._take(p_a, n, np.dtype("u1")), self._take(p_b, n, np.dtype("u1")), first

    def cigar_lift(self, cigar, chains, queries):
        """the coordinate map of the chains' CIGARs (nts_cigar_lift).  cigar [E] uint64 and chains, a CHAIN_DTYPE array: what cigar_build
        returns (entries need not be maximal runs); queries: a LIFT_QUERY_DTYPE array -- pos is an offset on side 0 (A) or 1 (B) of
        `chain`, 0 .. the chain's len_a or len_b, the end included.  Returns a LIFT_HIT_DTYPE array, one hit per query: pos = the offset
        on the other side, entry = the index into cigar of the entry that holds the query's position, off = how far into that entry,
        code = its kind (CIG_EQ, CIG_X: pos is the aligned base; CIG_DEL for side 0, CIG_INS for side 1: pos is the first base behind
        the gap); for the end of a chain (len_other, first + n_cig, 0, 0).  Entries that are no CIGAR of the chains' lengths and queries
        outside their chain are refused.  Exact and deterministic."""
        cg = np.ascontiguousarray(cigar, dtype=np.uint64)
        ch = np.ascontiguousarray(chains, dtype=CHAIN_DTYPE)
        qs = np.ascontiguousarray(queries, dtype=LIFT_QUERY_DTYPE)
        if cg.ndim != 1 or ch.ndim != 1 or qs.ndim != 1:
            raise ValueError("cigar_lift: a list of entries, a list of chain records and a list of queries")
        assert LIFT_QUERY_DTYPE.itemsize == ctypes.sizeof(_lib.LiftQuery) and LIFT_HIT_DTYPE.itemsize == ctypes.sizeof(_lib.LiftHit)
        assert CHAIN_DTYPE.itemsize == ctypes.sizeof(_lib.CigChain)
        hits = np.zeros(qs.size, dtype=LIFT_HIT_DTYPE)
        self.check(self.lib.nts_cigar_lift(self.h, cg.ctypes.data if cg.size else None, cg.size, ch.ctypes.data if ch.size else None, ch.size,
                                           qs.ctypes.data if qs.size else None, qs.size, hits.ctypes.data if hits.size else None), "nts_cigar_lift")
        return hits

    def cigar_lift_stats(self, cigar, chains, ranges):
        """the alignment counts of ranges of the chains' CIGARs (nts_cigar_lift_stats).  cigar and chains as for cigar_lift; ranges: a
        LIFT_RANGE_DTYPE array -- the bases lo .. hi - 1 (lo < hi <= the chain's len_a or len_b) of side 0 (A) or 1 (B) of `chain`.
        Returns a LIFT_STATS_DTYPE array, one record per range, over the chain's columns from the column of base lo to the column of
        base hi - 1: eq and x, the = and X columns; src_gap, the columns that consume the range's side only; oth_gap, the columns
        between the two that consume the other side only; src_gaps and oth_gaps, the maximal runs of either kind that hold a counted
        column; [oth_lo, oth_hi), the lifted span on the other side (eq + x + oth_gap long).  Entries that are no CIGAR of the chains'
        lengths and ranges outside their chain (an empty one included) are refused.  Exact and deterministic."""
        cg = np.ascontiguousarray(cigar, dtype=np.uint64)
        ch = np.ascontiguousarray(chains, dtype=CHAIN_DTYPE)
        rs = np.ascontiguousarray(ranges, dtype=LIFT_RANGE_DTYPE)
        if cg.ndim != 1 or ch.ndim != 1 or rs.ndim != 1:
            raise ValueError("cigar_lift_stats: a list of entries, a list of chain records and a list of ranges")
        assert LIFT_RANGE_DTYPE.itemsize == ctypes.sizeof(_lib.LiftRange) and LIFT_STATS_DTYPE.itemsize == ctypes.sizeof(_lib.LiftStats)
        assert CHAIN_DTYPE.itemsize == ctypes.sizeof(_lib.CigChain)
        stats = np.zeros(rs.size, dtype=LIFT_STATS_DTYPE)
        self.check(self.lib.nts_cigar_lift_stats(self.h, cg.ctypes.data if cg.size else None, cg.size, ch.ctypes.data if ch.size else None, ch.size,
                                                 rs.ctypes.data if rs.size else None, rs.size, stats.ctypes.data if stats.size else None),
                   "nts_cigar_lift_stats")
        return stats

    def cigar_lift_pairs(self, cigar, chains, links, pair_first, ranges):
        """one span and its counts per range and pair of chains (nts_cigar_lift_pairs).  cigar and chains as for cigar_lift; links: a
        LIFT_LINK_DTYPE array -- `chain` occupies [a0, a0 + len_a) on A and [b0, b0 + len_b) on B of its pair, in the pair's oriented
        offsets; pair_first [P + 1] uint64, nondecreasing from 0 to len(links): pair p's links, ascending without overlap on both sides;
        ranges: a PAIR_RANGE_DTYPE array -- the bases lo .. hi - 1 (lo < hi < 2^63) of side 0 (A) or 1 (B) of `pair`.  Returns a
        PAIR_STATS_DTYPE array, one record per range, over the pair's columns from the first to the last column that holds a base of
        the range: [src_lo, src_hi) the range clipped to the chains it reaches, [oth_lo, oth_hi) the lifted span, eq, x, src_gap,
        oth_gap the columns by kind, src_open and oth_open the bases between the chains that no column covers, src_gaps and oth_gaps
        the gap runs, link_lo .. link_hi the links reached, n_links their number -- 0, and every field 0, for a range that touches
        no chain.  Entries that are no CIGAR of the chains' lengths, links that are no placement of their chain and ranges of no pair
        are refused.  Exact and deterministic."""
        cg = np.ascontiguousarray(cigar, dtype=np.uint64)
        ch = np.ascontiguousarray(chains, dtype=CHAIN_DTYPE)
        lk = np.ascontiguousarray(links, dtype=LIFT_LINK_DTYPE)
        pf = np.ascontiguousarray(pair_first, dtype=np.uint64)
        rs = np.ascontiguousarray(ranges, dtype=PAIR_RANGE_DTYPE)
        if cg.ndim != 1 or ch.ndim != 1 or lk.ndim != 1 or pf.ndim != 1 or pf.size < 1 or rs.ndim != 1:
            raise ValueError("cigar_lift_pairs: a list of entries, of chain records, of links, of pairs' first links (one more than pairs) and of ranges")
        assert LIFT_LINK_DTYPE.itemsize == ctypes.sizeof(_lib.LiftLink) and PAIR_RANGE_DTYPE.itemsize == ctypes.sizeof(_lib.PairRange)
        assert PAIR_STATS_DTYPE.itemsize == ctypes.sizeof(_lib.PairStats) == 128 and CHAIN_DTYPE.itemsize == ctypes.sizeof(_lib.CigChain)
        stats = np.zeros(rs.size, dtype=PAIR_STATS_DTYPE)
        self.check(self.lib.nts_cigar_lift_pairs(self.h, cg.ctypes.data if cg.size else None, cg.size, ch.ctypes.data if ch.size else None, ch.size,
                                                 lk.ctypes.data if lk.size else None, lk.size, pf.ctypes.data, pf.size - 1,
                                                 rs.ctypes.data if rs.size else None, rs.size, stats.ctypes.data if stats.size else None),
                   "nts_cigar_lift_pairs")
        return stats

    def cigar_chain_blocks(self, cigar, chains, links, pair_first, text=True):
        """one liftover chain per pair of chains: the blocks of a UCSC chain file and their text (nts_cigar_chain_blocks).  cigar, chains,
        links and pair_first as for cigar_lift_pairs.  Returns (pairs, blocks) or, with text, (pairs, blocks, text, text_first): pairs a
        CHAIN_PAIR_DTYPE array, one record per pair -- [a0, a1) x [b0, b1) the liftover chain in the pair's oriented offsets from its
        first match column to behind its last, eq and x its = and X columns, blocks[first_block:first_block + n_blocks] its blocks, every
        field 0 for a pair without a match column; blocks a CHAIN_BLOCK_DTYPE array -- size, the columns of a maximal run of = / X with
        no gap of non-zero width inside, and dt, dq, the A and B bases of all gaps between it and the next block (D, I and the open
        stretches between linked chains), 0 for a pair's last block; text a uint8 array, per block the line "size\\tdt\\tdq\\n", for a
        pair's last block "size\\n"; pair p's lines are text[text_first[p]:text_first[p + 1]], text_first [P + 1] uint64.  The span and
        count identities of every pair are checked (RuntimeError).  Entries that are no CIGAR of the chains' lengths and links that are
        no placement of their chain are refused.  Exact and deterministic."""
        cg = np.ascontiguousarray(cigar, dtype=np.uint64)
        ch = np.ascontiguousarray(chains, dtype=CHAIN_DTYPE)
        lk = np.ascontiguousarray(links, dtype=LIFT_LINK_DTYPE)
        pf = np.ascontiguousarray(pair_first, dtype=np.uint64)
        if cg.ndim != 1 or ch.ndim != 1 or lk.ndim != 1 or pf.ndim != 1 or pf.size < 1:
            raise ValueError("cigar_chain_blocks: a list of entries, of chain records, of links and of pairs' first links (one more than pairs)")
        assert LIFT_LINK_DTYPE.itemsize == ctypes.sizeof(_lib.LiftLink) and CHAIN_DTYPE.itemsize == ctypes.sizeof(_lib.CigChain)
        assert CHAIN_BLOCK_DTYPE.itemsize == ctypes.sizeof(_lib.ChainBlock) == 24 and CHAIN_PAIR_DTYPE.itemsize == ctypes.sizeof(_lib.ChainPair) == 64
        pairs = np.zeros(pf.size - 1, dtype=CHAIN_PAIR_DTYPE)
        firsts = np.zeros(pf.size, dtype=np.uint64)
        p_blocks, p_text, n_blocks = c_vp(), c_vp(), u64()
        self.check(self.lib.nts_cigar_chain_blocks(self.h, cg.ctypes.data if cg.size else None, cg.size, ch.ctypes.data if ch.size else None, ch.size,
                                                   lk.ctypes.data if lk.size else None, lk.size, pf.ctypes.data, pf.size - 1,
                                                   pairs.ctypes.data if pairs.size else None, ctypes.byref(p_blocks), ctypes.byref(n_blocks),
                                                   ctypes.byref(p_text) if text else None, firsts.ctypes.data if text else None),
                   "nts_cigar_chain_blocks")
        blocks = self._take(p_blocks, n_blocks.value, CHAIN_BLOCK_DTYPE)
        chars = self._take(p_text, int(firsts[-1]), np.dtype("u1")) if text else None
        # the identities of docs/design/04_28_block_chain.md, per pair through prefix sums: no loop over blocks
        sums = np.zeros((3, blocks.size + 1), dtype=np.uint64)
        for row, name in zip(sums, ("size", "dt", "dq")):
            np.cumsum(blocks[name], out=row[1:])
        lo, hi = pairs["first_block"], pairs["first_block"] + pairs["n_blocks"]
        if blocks.size != int(pairs["n_blocks"].sum()) or (pairs.size and int(hi.max()) > blocks.size):
            raise RuntimeError("cigar_chain_blocks: the pairs' blocks do not tile the block list")
        size, dt, dq = (row[hi] - row[lo] for row in sums)
        is_last = np.zeros(blocks.size, dtype=bool)
        is_last[(hi[pairs["n_blocks"] > 0] - 1).astype(np.int64)] = True
        if not (np.array_equal(pairs["a1"] - pairs["a0"], size + dt) and np.array_equal(pairs["b1"] - pairs["b0"], size + dq) and
                np.array_equal(pairs["eq"] + pairs["x"], size) and bool((blocks["size"] > 0).all()) and
                np.array_equal((blocks["dt"] + blocks["dq"]) == 0, is_last)):
            raise RuntimeError("cigar_chain_blocks: a liftover chain breaks its span or count identities")
        return (pairs, blocks, chars, firsts) if text else (pairs, blocks)

    def timing(self, name):
        ms, n = ctypes.c_double(), u64()
        self.check(self.lib.nts_timing(self.h, name.encode(), ctypes.byref(ms), ctypes.byref(n)), "nts_timing")
        return ms.value, n.value

    def sketch_mode(self, mode="auto", prune_c=0):
        """'auto' (pruned when w >= 200; tiers below that where they pay), 'dense' (probe the filter for every k-mer) or 'pruned'
        (probe only k-mers whose hash is <= prune_c/w of the hash range; identical output)."""
        code = {"auto": 0, "dense": 1, "pruned": 2}[mode]
        self.check(self.lib.nts_sketch_mode(self.h, code, int(prune_c)), "nts_sketch_mode")
        self._sketch_mode = (mode, int(prune_c))

    def sketch_summary(self, mode=None):
        """Summary-first probing of sparse filters in the dense sketch (nts_sketch_summary): mode 'auto' / 'never' / 'no-lds'
        (summary, but no folded copy of the filter in LDS) / None (leave as is).  Returns the granule shift the last sketch call used (0: no summary)."""
        last = ctypes.c_uint32()
        code = {None: -1, "auto": 0, "never": 1, "no-lds": 2}[mode]
        self.check(self.lib.nts_sketch_summary(self.h, code, ctypes.byref(last)), "nts_sketch_summary")
        return last.value

    def sketch_select(self, impl="auto"):
        """candidate selection kernel of the pruned sketch (nts_sketch_select): 'auto', 'full' (full-width rolling) or 'hi' (upper
        halves rolled, also for assemblies in many pieces); same result"""
        self.check(self.lib.nts_sketch_select(self.h, {"auto": 0, "full": 1, "hi": 2}[impl]), "nts_sketch_select")

    def sketch_tiers(self, mode=None, x0=0.0, half_steps=False):
        """Tiered selection for filters that accept a few per cent of the k-mers (nts_sketch_tiers): mode 'auto' / 'never' / 'always'
        (wherever the kernel applies) / None (leave as is).  Returns (k-mers probed, rounds summed over the tiles, tiers planned) of
        the last sketch call; tiers == 0: it did not go that way.  Same result whichever way."""
        a, b, c = u64(), u64(), ctypes.c_uint32()
        code = {None: -1, "auto": 0, "never": 1, "always": 2}[mode]
        self.check(self.lib.nts_sketch_tiers(self.h, code, float(x0), int(bool(half_steps)), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
                   "nts_sketch_tiers")
        return a.value, b.value, c.value

    def bf_build_mode(self, mode="auto"):
        """How BloomFilter.insert sets the bits: 'auto' (partitioned streaming build for large genomes), 'atomic'
        (one atomic OR per k-mer) or 'binned' (partitioned whenever the filter layout allows); same filter."""
        self.check(self.lib.nts_bf_build_mode(self.h, {"auto": 0, "atomic": 1, "binned": 2}[mode]), "nts_bf_build_mode")

    def sketch_stats(self):
        "(accepted candidates, uncovered ranges, k-mers in them) of the last sketch call"
        a, b, c, d = u64(), u64(), u64(), ctypes.c_uint32()
        self.check(self.lib.nts_sketch_stats(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)),
                   "nts_sketch_stats")
        self.last_prune_c = d.value
        return a.value, b.value, c.value

    def path_stats(self):
        """dict(sketch_many_listed, bf_direct_indices, bf_list_fallback): the repeat / fragmentation paths the last sketch and the
        last partitioned Bloom build took (nts_path_stats)"""
        a, b, c = u64(), u64(), ctypes.c_uint32()
        self.check(self.lib.nts_path_stats(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "nts_path_stats")
        return {"sketch_many_listed": a.value, "bf_direct_indices": b.value, "bf_list_fallback": c.value}

    def bf_bin_last(self, idx32=False):
        """dict(bin1_workgroups, B1, log2_b2) of the last partitioned Bloom build: the workgroups of its first pass (0: it did not run)
        and the bucket geometry it was launched with (nts_bf_bin_last).  idx32=True: one key more, idx32 -- whether a residue's place
        in the level-1 array was a 32-bit index (nts_bf_bin_last_ex)."""
        a, b, c, d = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        self.check(self.lib.nts_bf_bin_last_ex(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)), "nts_bf_bin_last_ex")
        out = {"bin1_workgroups": a.value, "B1": b.value, "log2_b2": c.value}
        if idx32:
            out["idx32"] = d.value
        return out

    def bf_level_stats(self):
        """dict(sparse_level, accepted_kmers): whether the last BloomFilter.insert_and went the literal way over a running filter that
        is all but empty (every k-mer looked up, the bits that were hit kept) and how many k-mers it accepted (nts_bf_level_stats)"""
        a, b = ctypes.c_uint32(), u64()
        self.check(self.lib.nts_bf_level_stats(self.h, ctypes.byref(a), ctypes.byref(b)), "nts_bf_level_stats")
        return {"sparse_level": a.value, "accepted_kmers": b.value}

    VALU_KINDS = ["v_xor_b32", "v_alignbit_b32", "v_lshl_add_u64", "v_lshlrev_b64", "v_mul_lo_u32", "v_mad_u64_u32",
                  "v_add_co_u32+v_addc_co_u32", "v_xor_b32 (dependent chain)", "v_add3_u32", "v_cmp_ge_u32+v_addc_co_u32",
                  "roll31 step (9 instructions)"]

    def bench_valu(self, kind, waves_per_simd=4, iters=20000):
        """Issue-rate microbenchmark of one integer VALU instruction (nts_bench_valu): dict with the shader cycles a SIMD
        spends per wave-instruction and the wave-instructions per second per CU the wall time gives."""
        ms, cyc, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        k = self.VALU_KINDS.index(kind) if isinstance(kind, str) else int(kind)
        self.check(self.lib.nts_bench_valu(self.h, k, int(waves_per_simd), int(iters), ctypes.byref(ms), ctypes.byref(cyc),
                                           ctypes.byref(n)), "nts_bench_valu")
        per_cu = 4 * waves_per_simd * n.value / (ms.value * 1e-3)
        return {"instruction": self.VALU_KINDS[k], "waves_per_simd": int(waves_per_simd), "wall_ms": round(ms.value, 4),
                "cycles_per_wave_instr_per_simd": round(cyc.value, 3), "wave_instr_per_s_per_cu": per_cu,
                # 4 SIMDs per CU, each issuing one wave-instruction per `cycles`: the clock the two figures imply
                "implied_clock_GHz": round(per_cu * cyc.value / 4 / 1e9, 3)}

    def set_graph_budget(self, nbytes):
        """Bytes the graph build's per-slice scratch may take on this context (nts_graph_budget); 0 = automatic (free device memory).
        A build whose sorts do not fit runs in hash-range slices; same graph."""
        self.check(self.lib.nts_graph_budget(self.h, int(nbytes)), "nts_graph_budget")

    def graph_last_plan(self):
        "dict(v_slices, e_slices, scratch_peak, oversize) of the last graph build on this context (nts_graph_last_plan)"
        v, e, o, p = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32(), u64()
        self.check(self.lib.nts_graph_last_plan(self.h, ctypes.byref(v), ctypes.byref(e), ctypes.byref(p), ctypes.byref(o)),
                   "nts_graph_last_plan")
        return {"v_slices": v.value, "e_slices": e.value, "scratch_peak": p.value, "oversize": o.value}

    def mem_stats(self):
        """Device memory of the library's allocations in this process: dict(live, peak, device_used, device_total) in bytes
        (nts_mem_stats; `peak` is the high-water mark since the last mem_reset_peak())."""
        a, b, c, d = u64(), u64(), u64(), u64()
        self.check(self.lib.nts_mem_stats(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)), "nts_mem_stats")
        return {"live": a.value, "peak": b.value, "device_used": c.value, "device_total": d.value}

    def alloc_stats(self):
        "(hipMalloc / hipFree calls the library has made in this process, host milliseconds spent in them): nts_alloc_stats"
        n, ms = u64(), ctypes.c_double()
        self.lib.nts_alloc_stats(ctypes.byref(n), ctypes.byref(ms))
        return n.value, ms.value

    def mem_trim(self):
        "every block of the library's allocation cache back to the driver; bytes released (nts_mem_trim)"
        return int(self.lib.nts_mem_trim())

    def mem_cache_stats(self):
        "(bytes the allocation cache holds, allocations it has served): nts_mem_cache_stats"
        a, b = u64(), u64()
        self.lib.nts_mem_cache_stats(ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value

    def mem_reset_peak(self):
        self.lib.nts_mem_reset_peak()

    def mem_reserve(self, nbytes):
        "one driver allocation of `nbytes` kept for the allocations to come (nts_mem_reserve); returns the bytes reserved"
        got = u64()
        self.check(self.lib.nts_mem_reserve(self.device, int(nbytes), ctypes.byref(got)), "nts_mem_reserve")
        return got.value

    def mem_reserve_async(self, nbytes):
        """the same on a thread of its own (the call spends its time in the driver, outside the interpreter lock): a run starts it
        before it opens its first file; .join() returns the bytes reserved (0 when the driver refused: the run then allocates as it goes)"""
        import threading
        box = {"got": 0}

        def work():
            try:
                box["got"] = self.mem_reserve(nbytes)
            except Exception:
                box["got"] = 0
        th = threading.Thread(target=work, name="nts_mem_reserve", daemon=True)
        th.start()

        class _Pending:
            def join(self_inner):
                th.join()
                return box["got"]
        return _Pending()

    def mem_events(self):
        "process-wide allocation counters (nts_mem_events) as a dict; take differences around a stage (mem_events_since)"
        return mem_events(self.lib)

    def mem_events_since(self, before):
        return mem_events_since(self.lib, before)

    def trim_ingest(self):
        "give back the FASTA ingest's workspaces (the raw image of the largest file, pinned staging): nts_ingest_trim"
        self.check(self.lib.nts_ingest_trim(self.h), "nts_ingest_trim")

    def trim_bf_build(self):
        "the Bloom build's bucket arrays back to the allocation cache (the run's last filter is made): nts_bf_build_trim"
        self.check(self.lib.nts_bf_build_trim(self.h), "nts_bf_build_trim")

    def close(self):
        if self.h:
            self.lib.nts_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


BF_ROUNDING = {"up": 0, "down": 1, "none": 2}


def bf_size_bytes(genome_bp, fpr, rounding="up"):
    """(approx_bytes, ctor_bytes): src/ntsynt_make_common_bf.cpp:28-40 + btllib ctor rounding.  `rounding` selects the
    constructor's rule ('up' = ceil(bytes / 8.0) * 8, recalled from btllib; 'down' and 'none' are the alternatives a
    reader of btllib's source can switch to: SURVEY.md 8(c) u1)."""
    a, c = u64(), u64()
    rc = _lib.load().nts_bf_size_bytes_ex(int(genome_bp), float(fpr), BF_ROUNDING[rounding], ctypes.byref(a), ctypes.byref(c))
    if rc != 0:
        raise NtsError("nts_bf_size_bytes: bad arguments")
    return a.value, c.value


BF_BIN_PLAN_FIELDS = ("F", "log2_b2", "B2", "B1", "n_final", "cap1", "cap2", "tiles", "tiles2", "idx32")


def bf_bin_plan(n_valid, nbytes, k=24, forced=True, and_mode=False):
    """The geometry of the partitioned Bloom build for n_valid k-mers and a filter of nbytes bytes (nts_bf_bin_plan, a host function:
    no GPU): a dict of BF_BIN_PLAN_FIELDS, or None when the partitioned build does not apply."""
    out = (u64 * len(BF_BIN_PLAN_FIELDS))()
    rc = _lib.load().nts_bf_bin_plan(int(n_valid), int(nbytes), int(k), int(bool(forced)), int(bool(and_mode)), out)
    if rc not in (0, 1):
        raise NtsError("nts_bf_bin_plan: bad arguments")
    return dict(zip(BF_BIN_PLAN_FIELDS, (int(x) for x in out))) if rc == 0 else None


class Genome:
    """A FASTA resident in HBM.  names: record ids; seq: uint8 array of the concatenated bases."""

    def __init__(self, ctx, names, seq, rec_off, rec_len):
        self.ctx = ctx
        self.names = list(names)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        self.rec_off = np.ascontiguousarray(rec_off, dtype=np.uint64)
        self.rec_len = np.ascontiguousarray(rec_len, dtype=np.uint64)
        self.n_bytes = int(seq.size)
        h = c_vp()
        ctx.check(ctx.lib.nts_genome_upload(ctx.h, seq.ctypes.data, seq.size,
                                            self.rec_off.ctypes.data_as(_lib.c_u64p),
                                            self.rec_len.ctypes.data_as(_lib.c_u64p),
                                            len(self.names), ctypes.byref(h)), "nts_genome_upload")
        self.h = h

    @classmethod
    def synth(cls, ctx, total_bp, n_contigs, seed_ancestor, seed_genome, substitution_rate):
        """Synthetic genome generated in HBM (bench / scale tests): relatives share seed_ancestor."""
        g = cls.__new__(cls)
        g.ctx = ctx
        per = int(total_bp) // int(n_contigs)
        g.names = [f"chr{i + 1}" for i in range(n_contigs)]
        g.rec_len = np.full(n_contigs, per, dtype=np.uint64)
        g.rec_off = (np.arange(n_contigs, dtype=np.uint64) * np.uint64(per)).astype(np.uint64)
        g.n_bytes = per * int(n_contigs)
        h = c_vp()
        ctx.check(ctx.lib.nts_genome_synth(ctx.h, int(total_bp), int(n_contigs), int(seed_ancestor), int(seed_genome),
                                           float(substitution_rate), ctypes.byref(h)), "nts_genome_synth")
        g.h = h
        return g

    @classmethod
    def synth_plan(cls, ctx, plan, seed_ancestor, seed_genome, substitution_rate, rep=None, names=None):
        """Synthetic genome with structural events generated in HBM (nts_genome_synth_plan[_ex]): `plan` = (record lengths,
        pieces) from ntsynt_amd.synth.structural_plan / realistic_plan; relatives share seed_ancestor and the ancestor's layout.
        rep: dict of nts_synth_repeats fields (synth.REPEATS) -- the assembly-like ancestor with interspersed repeats and
        satellite arrays."""
        rec_len, pieces = plan[0], plan[1]
        g = cls.__new__(cls)
        g.ctx = ctx
        rec_len = np.ascontiguousarray(rec_len, dtype=np.uint64)
        pieces = np.ascontiguousarray(pieces)
        assert pieces.dtype.itemsize == 32
        g.names = list(names) if names is not None else [f"chr{i + 1}" for i in range(rec_len.size)]
        g.rec_len = rec_len
        g.rec_off = np.concatenate(([0], np.cumsum(rec_len[:-1]))).astype(np.uint64)
        g.n_bytes = int(rec_len.sum())
        h = c_vp()
        rp = None
        if rep is not None:
            rp = _lib.SynthRepeats(**{k_: int(v) for k_, v in rep.items()})
        ctx.check(ctx.lib.nts_genome_synth_plan_ex(ctx.h, rec_len.size, rec_len.ctypes.data, pieces.size, pieces.ctypes.data,
                                                   int(seed_ancestor), int(seed_genome), float(substitution_rate),
                                                   ctypes.byref(rp) if rp is not None else None, ctypes.byref(h)),
                  "nts_genome_synth_plan")
        g.h = h
        return g

    @classmethod
    def concat(cls, ctx, parts):
        """The batch of resident genomes `parts` as one resident genome (nts_genome_concat, a device-to-device copy):
        record ids of part p start at rec_base[p].  One sketch of the batch replaces one sketch per part --
        split_minimizers() takes the list apart again."""
        g = cls.__new__(cls)
        g.ctx = ctx
        g.names = [n for p in parts for n in p.names]
        g.rec_base = np.concatenate(([0], np.cumsum([len(p.names) for p in parts]))).astype(np.int64)
        sizes = np.array([p.n_bytes for p in parts], dtype=np.uint64)
        g.n_bytes = int(sizes.sum())
        starts = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.uint64)
        g.rec_off = np.concatenate([p.rec_off + s for p, s in zip(parts, starts)]).astype(np.uint64)
        g.rec_len = np.concatenate([p.rec_len for p in parts]).astype(np.uint64)
        arr = (c_vp * len(parts))(*[p.h for p in parts])
        h = c_vp()
        ctx.check(ctx.lib.nts_genome_concat(ctx.h, len(parts), arr, ctypes.byref(h)), "nts_genome_concat")
        g.h = h
        return g

    def slice(self, rec0, rec1, ctx=None):
        """Records [rec0, rec1) as a resident genome of their own (nts_genome_slice): the shard one rank of this genome's group
        works on when there are fewer genomes than GPUs; record r of the slice is record rec0 + r here."""
        ctx = ctx or self.ctx
        g = Genome.__new__(Genome)
        g.ctx = ctx
        g.names = self.names[rec0:rec1]
        g.rec_len = np.ascontiguousarray(self.rec_len[rec0:rec1], dtype=np.uint64)
        g.rec_off = (np.concatenate(([0], np.cumsum(g.rec_len[:-1]))) if rec1 > rec0 else np.zeros(0)).astype(np.uint64)
        g.n_bytes = int(g.rec_len.sum())
        g.rec0 = int(rec0)
        h = c_vp()
        ctx.check(ctx.lib.nts_genome_slice(ctx.h, self.h, int(rec0), int(rec1), ctypes.byref(h)), "nts_genome_slice")
        g.h = h
        return g

    def split_minimizers(self, h1, rec, pos):
        """(h1, rec, pos) of a sketch of a concat() batch -> one (h1, rec, pos) per part, record ids local to the part
        (the list is in (record, position) order, so each part is a slice)."""
        cut = np.searchsorted(rec, self.rec_base.astype(rec.dtype))
        return [(h1[a:b], rec[a:b] - rec.dtype.type(base), pos[a:b])
                for a, b, base in zip(cut[:-1], cut[1:], self.rec_base[:-1])]

    def download(self, offset, length):
        "upper-case ASCII of bases [offset, offset+length) of the concatenated records"
        out = np.empty(int(length), dtype=np.uint8)
        self.ctx.check(self.ctx.lib.nts_genome_download(self.ctx.h, self.h, int(offset), int(length), out.ctypes.data),
                       "nts_genome_download")
        return out

    @property
    def total_bp(self):
        return int(self.ctx.lib.nts_genome_bases(self.h))

    def valid_kmers(self, k):
        n = u64()
        self.ctx.check(self.ctx.lib.nts_genome_valid_kmers(self.ctx.h, self.h, k, ctypes.byref(n)), "valid_kmers")
        return n.value

    def hash_all(self, k):
        "canonical h0 of every valid k-mer in (record, position) order (test hook, row B1)"
        p, n = _lib.c_u64p(), u64()
        self.ctx.check(self.ctx.lib.nts_hash_all(self.ctx.h, self.h, k, ctypes.byref(p), ctypes.byref(n)), "nts_hash_all")
        out = np.ctypeslib.as_array(p, shape=(max(n.value, 1),))[:n.value].copy()
        self.ctx.lib.nts_free(p)
        return out

    def minhash(self, k, s):
        """bottom-s MinHash sketch (nts_minhash): the s smallest distinct canonical h0 over the valid k-mers, ascending --
        exactly np.unique(hash_all(k))[:s] without the sentinel 2^64 - 1 (fewer than s if there are fewer distinct k-mers)"""
        out = np.empty(max(int(s), 1), dtype=np.uint64)
        n = _lib.u32()
        self.ctx.check(self.ctx.lib.nts_minhash(self.ctx.h, self.h, int(k), int(s), out.ctypes.data_as(_lib.c_u64p), ctypes.byref(n)),
                       "nts_minhash")
        return out[:n.value].copy()

    def minhash_intervals(self, intervals, k, s):
        """bottom-s sketches of many intervals in one sweep (nts_minhash_intervals).  intervals: (rec, start, end) rows -- the valid
        k-mers wholly inside [start, end) of record rec, end clipped to the record.  Returns (sketches [n, s] uint64 -- row i holds
        counts[i] hashes, ascending, distinct --, counts [n] uint32, n_kmers [n] uint64)."""
        rows = np.asarray(intervals, dtype=np.uint64).reshape(-1, 3)
        n, s = rows.shape[0], int(s)
        iv = np.zeros(n, dtype=np.dtype([("rec", "<u4"), ("start", "<u8"), ("end", "<u8")], align=True))
        assert iv.dtype.itemsize == ctypes.sizeof(Interval)
        iv["rec"], iv["start"], iv["end"] = rows[:, 0], rows[:, 1], rows[:, 2]
        out = np.zeros((n, max(s, 1)), dtype=np.uint64)
        counts = np.zeros(n, dtype=np.uint32)
        n_kmers = np.zeros(n, dtype=np.uint64)
        self.ctx.check(self.ctx.lib.nts_minhash_intervals(self.ctx.h, self.h, int(k), s, ctypes.cast(iv.ctypes.data, ctypes.POINTER(Interval)), n,
                                                          out.ctypes.data, counts.ctypes.data, n_kmers.ctypes.data), "nts_minhash_intervals")
        return out, counts, n_kmers

    @staticmethod
    def _interval_array(intervals):
        "(rec, start, end) rows in nts_interval's layout"
        rows = np.asarray(intervals, dtype=np.uint64).reshape(-1, 3)
        iv = np.zeros(rows.shape[0], dtype=np.dtype([("rec", "<u4"), ("start", "<u8"), ("end", "<u8")], align=True))
        assert iv.dtype.itemsize == ctypes.sizeof(Interval)
        iv["rec"], iv["start"], iv["end"] = rows[:, 0], rows[:, 1], rows[:, 2]
        return iv

    def valid_bases(self, intervals):
        "per interval its A/C/G/T bases (nts_genome_valid_bases: host arithmetic over the genome's valid stretches); [n] uint64"
        iv = self._interval_array(intervals)
        out = np.zeros(iv.size, dtype=np.uint64)
        self.ctx.check(self.ctx.lib.nts_genome_valid_bases(self.ctx.h, self.h, ctypes.cast(iv.ctypes.data, ctypes.POINTER(Interval)), iv.size,
                                                           out.ctypes.data), "nts_genome_valid_bases")
        return out

    def bf_count_intervals(self, bf, intervals, k):
        """per interval the valid k-mers wholly inside it and how many of them the Bloom filter `bf` holds (nts_bf_count_intervals):
        intervals as in minhash_intervals; returns (kmers [n] uint64, hits [n] uint64), exact"""
        iv = self._interval_array(intervals)
        n = iv.size
        kmers = np.zeros(n, dtype=np.uint64)
        hits = np.zeros(n, dtype=np.uint64)
        self.ctx.check(self.ctx.lib.nts_bf_count_intervals(self.ctx.h, self.h, int(k), bf.h, ctypes.cast(iv.ctypes.data, ctypes.POINTER(Interval)), n,
                                                           kmers.ctypes.data, hits.ctypes.data), "nts_bf_count_intervals")
        return kmers, hits

    def bf_sample_intervals(self, bf, intervals, k, rate):
        """a thin sample of the k-mers of the intervals that the Bloom filter `bf` holds (nts_bf_sample_intervals): those with
        h0 <= (2^64 - 1) // rate.  intervals as in minhash_intervals.  Returns (records, counts): a SAMPLE_DTYPE array in interval
        order, then k-mer order (iv = the interval's row, off = the k-mer's position minus the interval's clipped start), and the
        records per interval [n] uint64.  Exact and deterministic."""
        iv = self._interval_array(intervals)
        n = iv.size
        counts = np.zeros(n, dtype=np.uint64)
        p, m = c_vp(), u64()
        self.ctx.check(self.ctx.lib.nts_bf_sample_intervals(self.ctx.h, self.h, int(k), bf.h, int(rate), ctypes.cast(iv.ctypes.data, ctypes.POINTER(Interval)),
                                                            n, counts.ctypes.data, ctypes.byref(p), ctypes.byref(m)), "nts_bf_sample_intervals")
        out = np.empty(m.value, dtype=SAMPLE_DTYPE)
        if m.value:
            ctypes.memmove(out.ctypes.data, p.value, out.nbytes)
        self.ctx.lib.nts_free(p)
        return out, counts

    def sample_intervals(self, intervals, k, rate):
        """bf_sample_intervals without a filter (nts_sample_intervals): every valid k-mer wholly inside an interval with
        h0 <= (2^64 - 1) // rate, whatever holds it.  The same (records, counts), exact and deterministic."""
        iv = self._interval_array(intervals)
        n = iv.size
        counts = np.zeros(n, dtype=np.uint64)
        p, m = c_vp(), u64()
        self.ctx.check(self.ctx.lib.nts_sample_intervals(self.ctx.h, self.h, int(k), int(rate), ctypes.cast(iv.ctypes.data, ctypes.POINTER(Interval)), n,
                                                         counts.ctypes.data, ctypes.byref(p), ctypes.byref(m)), "nts_sample_intervals")
        out = np.empty(m.value, dtype=SAMPLE_DTYPE)
        if m.value:
            ctypes.memmove(out.ctypes.data, p.value, out.nbytes)
        self.ctx.lib.nts_free(p)
        return out, counts

    def hset_sample_intervals(self, hset, intervals, k, rate):
        """bf_sample_intervals with the exact hash set `hset` (HashSet) in place of the filter (nts_hset_sample_intervals): the k-mers of
        the intervals with h0 <= (2^64 - 1) // rate whose h0 is a member.  The same (records, counts), exact and deterministic."""
        iv = self._interval_array(intervals)
        n = iv.size
        counts = np.zeros(n, dtype=np.uint64)
        p, m = c_vp(), u64()
        self.ctx.check(self.ctx.lib.nts_hset_sample_intervals(self.ctx.h, self.h, int(k), hset.h, int(rate), ctypes.cast(iv.ctypes.data, ctypes.POINTER(Interval)),
                                                              n, counts.ctypes.data, ctypes.byref(p), ctypes.byref(m)), "nts_hset_sample_intervals")
        out = np.empty(m.value, dtype=SAMPLE_DTYPE)
        if m.value:
            ctypes.memmove(out.ctypes.data, p.value, out.nbytes)
        self.ctx.lib.nts_free(p)
        return out, counts

    def hset_count_intervals(self, hset, counts, intervals, k, rate):
        """for every k-mer of the intervals with h0 <= (2^64 - 1) // rate whose h0 is a member of `hset` (HashSet), 1 to its count in
        `counts` (HashCounts of that set) (nts_hset_count_intervals).  intervals as in minhash_intervals; a k-mer counts once per
        interval that holds it; counts accumulate until counts.clear().  Returns the hits per interval [n] uint64."""
        iv = self._interval_array(intervals)
        n = iv.size
        hits = np.zeros(n, dtype=np.uint64)
        self.ctx.check(self.ctx.lib.nts_hset_count_intervals(self.ctx.h, self.h, int(k), hset.h, counts.h, int(rate),
                                                             ctypes.cast(iv.ctypes.data, ctypes.POINTER(Interval)), n, hits.ctypes.data),
                       "nts_hset_count_intervals")
        return hits

    def hset_sample_intervals_capped(self, hset, counts, cap, intervals, k, rate):
        """hset_sample_intervals that keeps a k-mer only when its count in `counts` (HashCounts of `hset`) lies in 1..cap
        (nts_hset_sample_intervals_capped).  The counter is only read.  The same (records, per-interval counts), exact and
        deterministic."""
        iv = self._interval_array(intervals)
        n = iv.size
        per_iv = np.zeros(n, dtype=np.uint64)
        p, m = c_vp(), u64()
        self.ctx.check(self.ctx.lib.nts_hset_sample_intervals_capped(self.ctx.h, self.h, int(k), hset.h, counts.h, int(cap), int(rate),
                                                                     ctypes.cast(iv.ctypes.data, ctypes.POINTER(Interval)), n, per_iv.ctypes.data,
                                                                     ctypes.byref(p), ctypes.byref(m)), "nts_hset_sample_intervals_capped")
        out = np.empty(m.value, dtype=SAMPLE_DTYPE)
        if m.value:
            ctypes.memmove(out.ctypes.data, p.value, out.nbytes)
        self.ctx.lib.nts_free(p)
        return out, per_iv

    def free(self):
        if self.h:
            self.ctx.lib.nts_genome_free(self.ctx.h, self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class HashSet:
    """An exact set of 64-bit hashes in HBM (nts_hset_build): what Genome.hset_sample_intervals probes.  After free() every call with
    it is refused (the handle is NULL)."""

    def __init__(self, ctx, values):
        "values: any array of uint64, duplicates allowed, empty allowed"
        self.ctx = ctx
        v = np.ascontiguousarray(values, dtype=np.uint64).ravel()
        h = c_vp()
        ctx.check(ctx.lib.nts_hset_build(ctx.h, v.ctypes.data if v.size else None, v.size, ctypes.byref(h)), "nts_hset_build")
        self.h = h

    def contains(self, values):
        "[n] bool: which of the values are members (nts_hset_contains)"
        v = np.ascontiguousarray(values, dtype=np.uint64).ravel()
        out = np.zeros(v.size, dtype=np.uint8)
        self.ctx.check(self.ctx.lib.nts_hset_contains(self.ctx.h, self.h, v.ctypes.data if v.size else None, v.size, out.ctypes.data if v.size else None),
                       "nts_hset_contains")
        return out.astype(bool)

    def free(self):
        if self.h:
            self.ctx.lib.nts_hset_free(self.ctx.h, self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class HashCounts:
    """Per member of a HashSet, how often it was seen: 32-bit counts in HBM beside the set's table (nts_hcount_create), all zero at
    first.  Genome.hset_count_intervals and add() add to them; they are read by key.  Free it before its set.  After free() every
    call with it is refused (the handle is NULL)."""

    def __init__(self, ctx, hset):
        self.ctx, self.hset = ctx, hset
        h = c_vp()
        ctx.check(ctx.lib.nts_hcount_create(ctx.h, hset.h, ctypes.byref(h)), "nts_hcount_create")
        self.h = h

    def add(self, values):
        "every value that is a member adds 1 to its count; the others add nothing (nts_hcount_add)"
        v = np.ascontiguousarray(values, dtype=np.uint64).ravel()
        self.ctx.check(self.ctx.lib.nts_hcount_add(self.ctx.h, self.hset.h, self.h, v.ctypes.data if v.size else None, v.size), "nts_hcount_add")

    def read(self, values):
        "[n] uint32: the count of each value, 0 for one that is not a member (nts_hcount_read)"
        v = np.ascontiguousarray(values, dtype=np.uint64).ravel()
        out = np.zeros(v.size, dtype=np.uint32)
        self.ctx.check(self.ctx.lib.nts_hcount_read(self.ctx.h, self.hset.h, self.h, v.ctypes.data if v.size else None, v.size,
                                                    out.ctypes.data if v.size else None), "nts_hcount_read")
        return out

    def clear(self):
        "every count back to zero (nts_hcount_clear)"
        self.ctx.check(self.ctx.lib.nts_hcount_clear(self.ctx.h, self.h), "nts_hcount_clear")

    def free(self):
        if self.h:
            self.ctx.lib.nts_hcount_free(self.ctx.h, self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class BloomFilter:
    """btllib::KmerBloomFilter(bytes, 1, k) stand-in, bit array in HBM."""

    def __init__(self, ctx, nbytes, k, world=1, ones=False):
        """world > 1: allocation laid out for Comm.allreduce_and (nts_bf_create_sharded); ones: all bits set, the
        identity of AND for a rank that owns no genome."""
        self.ctx, self.k = ctx, k
        h = c_vp()
        if world > 1:
            ctx.check(ctx.lib.nts_bf_create_sharded(ctx.h, int(nbytes), int(world), ctypes.byref(h)), "nts_bf_create_sharded")
        else:
            ctx.check(ctx.lib.nts_bf_create(ctx.h, int(nbytes), ctypes.byref(h)), "nts_bf_create")
        self.h = h
        self.bytes = int(nbytes)
        if ones:
            ctx.check(ctx.lib.nts_bf_fill_ones(ctx.h, h), "nts_bf_fill_ones")

    def insert(self, genome):
        "bf->insert(record.seq) for every record (cpp:128-131)"
        self.ctx.check(self.ctx.lib.nts_bf_insert(self.ctx.h, self.h, genome.h, self.k), "nts_bf_insert")

    def insert_and(self, genome):
        """one cascade level (cpp:134-160) in place: self &= the filter of `genome`, fused into the build's last pass
        (nts_bf_insert_and) -- what clear + insert into a second filter + and_ give, without the second filter"""
        self.ctx.check(self.ctx.lib.nts_bf_insert_and(self.ctx.h, self.h, genome.h, self.k), "nts_bf_insert_and")

    def cascade_from(self, prev, genome):
        "`if prev.contains(h): self.insert(h)` over every k-mer of genome (cpp:145-153)"
        self.ctx.check(self.ctx.lib.nts_bf_cascade(self.ctx.h, prev.h, self.h, genome.h, self.k), "nts_bf_cascade")

    def insert_repeats_of(self, genome, genome_bf):
        """self = the repeat filter: every k-mer of `genome` whose bit is set in genome_bf already sets its bit here, the others set
        it in genome_bf (bin/ntsynt_make_repeat_bfs.py:56-67)"""
        self.ctx.check(self.ctx.lib.nts_bf_insert_repeats(self.ctx.h, genome_bf.h, self.h, genome.h, self.k), "nts_bf_insert_repeats")

    def and_(self, other):
        self.ctx.check(self.ctx.lib.nts_bf_and(self.ctx.h, self.h, other.h), "nts_bf_and")

    def clear(self):
        self.ctx.check(self.ctx.lib.nts_bf_clear(self.ctx.h, self.h), "nts_bf_clear")

    def popcount(self):
        n = u64()
        self.ctx.check(self.ctx.lib.nts_bf_popcount(self.ctx.h, self.h, ctypes.byref(n)), "nts_bf_popcount")
        return n.value

    def get_fpr(self):
        "occupancy (one hash function), what the reference prints at cpp:132,154,162"
        return self.popcount() / float(self.bytes * 8)

    def bench_random_probe(self, n_probes, repeats=3):
        "microbenchmark: average ms for n_probes random single-bit reads (no hashing)"
        ms, hits = ctypes.c_double(), u64()
        self.ctx.check(self.ctx.lib.nts_bench_random_probe(self.ctx.h, self.h, int(n_probes), int(repeats), ctypes.byref(ms),
                                                           ctypes.byref(hits)), "nts_bench_random_probe")
        return ms.value

    def device_ptr(self):
        return int(self.ctx.lib.nts_bf_device_ptr(self.h))

    def to_numpy(self):
        out = np.empty(self.bytes, dtype=np.uint8)
        self.ctx.check(self.ctx.lib.nts_bf_download(self.ctx.h, self.h, out.ctypes.data, self.bytes), "nts_bf_download")
        return out

    def save(self, path, header=b"", threads=0):
        "bf->save(path): header bytes + the bit array streamed out of HBM into the file (nts_bf_save), no host copy"
        self.ctx.check(self.ctx.lib.nts_bf_save(self.ctx.h, self.h, os.fsencode(path), header, len(header), int(threads)), "nts_bf_save")

    def from_numpy(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint8)
        self.ctx.check(self.ctx.lib.nts_bf_upload(self.ctx.h, self.h, arr.ctypes.data, arr.size), "nts_bf_upload")

    def free(self):
        if self.h:
            self.ctx.lib.nts_bf_free(self.ctx.h, self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Comm:
    """RCCL communicator of the multi-GPU path, one rank per GPU (nts_comm_*).  `exchange_id(id_or_None) -> id` hands the
    128-byte id made on rank 0 to every rank (torch.distributed's store in this package; any launcher would do)."""

    def __init__(self, ctx, world, rank, exchange_id):
        self.ctx, self.world, self.rank = ctx, int(world), int(rank)
        ident = None
        if rank == 0:
            buf = (ctypes.c_uint8 * 128)()
            if ctx.lib.nts_comm_unique_id(buf) != 0:
                raise NtsError("nts_comm_unique_id failed: librccl could not be loaded")
            ident = bytes(buf)
        ident = exchange_id(ident)
        h = c_vp()
        raw = (ctypes.c_uint8 * 128).from_buffer_copy(ident)
        ctx.check(ctx.lib.nts_comm_init(ctx.h, raw, self.world, self.rank, ctypes.byref(h)), "nts_comm_init")
        self.h = h

    @classmethod
    def from_torch(cls, ctx):
        "communicator over the ranks of torch.distributed's default group (used only to pass the id around)"
        import torch.distributed as dist

        def exchange(ident):
            box = [ident]
            dist.broadcast_object_list(box, src=0)
            return box[0]
        return cls(ctx, dist.get_world_size(), dist.get_rank(), exchange)

    def allreduce_and(self, bf):
        "exchange 1: bf &= every other rank's filter, in place (bf from BloomFilter(..., world=N))"
        self.ctx.check(self.ctx.lib.nts_bf_allreduce_and(self.ctx.h, bf.h, self.h), "nts_bf_allreduce_and")

    def allreduce_groups(self, bf, group_of):
        """exchange 1 with genomes sharded over groups of ranks: bf = AND over groups of (OR over the filters of the group's ranks),
        in place; group_of[r] = group (genome) of rank r (nts_bf_allreduce_groups)"""
        arr = (ctypes.c_int32 * self.world)(*[int(g) for g in group_of])
        self.ctx.check(self.ctx.lib.nts_bf_allreduce_groups(self.ctx.h, bf.h, self.h, arr, max(group_of) + 1), "nts_bf_allreduce_groups")

    def allreduce_parts(self, filters, slot_group, n_slots, n_groups):
        """exchange 1 with a family's records shared out by bases (pipeline.partition_plan): this rank's `filters` (one per genome its
        range touches, all from BloomFilter(..., world=N); filters[0] receives the result; a rank without records passes one filter),
        slot_group[r][s] = genome of rank r's s-th filter or -1 (nts_bf_allreduce_parts)"""
        flat = [int(g) for row in slot_group for g in (list(row) + [-1] * (n_slots - len(row)))]
        arr = (ctypes.c_int32 * len(flat))(*flat)
        hs = (c_vp * len(filters))(*[f.h for f in filters])
        self.ctx.check(self.ctx.lib.nts_bf_allreduce_parts(self.ctx.h, hs, len(filters), self.h, int(n_slots), arr, int(n_groups)),
                       "nts_bf_allreduce_parts")

    def rccl_ranks(self):
        "ranks of the communicator as the library sees it (nts_comm_world)"
        return int(self.ctx.lib.nts_comm_world(self.h))

    def last_sparse(self):
        "True if the last all-reduce gathered set-bit indices instead of the reduced chunks"
        return bool(self.ctx.lib.nts_comm_last_sparse(self.ctx.h))

    def last_exchange2(self):
        "the last exchange 2 of this context: dict(packed_bytes, unpacked_bytes, sent_bytes) -- nts_comm_last_exchange2"
        a, b, c = u64(), u64(), u64()
        self.ctx.lib.nts_comm_last_exchange2(self.ctx.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        return {"packed_bytes": a.value, "unpacked_bytes": b.value, "sent_bytes": c.value}

    def allgather_minimizers(self, local, local_ids, n_total, slots=0):
        """exchange 2: the ranks' Minimizers -> [Minimizers of list g for g in range(n_total)], resident in HBM; slots: lists a rank may
        hold (0: ceil(n_total / world))"""
        return allgather_minimizers(self.ctx, self, local, local_ids, n_total, slots)

    def close(self):
        if self.h:
            self.ctx.lib.nts_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def allgather_minimizers(ctx, comm, local, local_ids, n_total, slots=0):
    "nts_mx_allgather_ex; comm None = one rank (the lists are copied into fresh handles)"
    n = len(local)
    arr = (c_vp * max(n, 1))(*[m.h for m in local])
    ids = (ctypes.c_uint32 * max(n, 1))(*[int(i) for i in local_ids])
    out = (c_vp * int(n_total))()
    ctx.check(ctx.lib.nts_mx_allgather_ex(ctx.h, comm.h if comm is not None else None, n, arr, ids, int(n_total), int(slots), out),
              "nts_mx_allgather")
    return [Minimizers(ctx, c_vp(out[g])) for g in range(int(n_total))]


class Minimizers:
    """Device-resident minimizer list of one genome, in (record, position) order."""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    def __len__(self):
        return int(self.ctx.lib.nts_mx_count(self.h))

    def to_numpy(self):
        n = len(self)
        h1 = np.empty(n, dtype=np.uint64)
        rec = np.empty(n, dtype=np.uint32)
        pos = np.empty(n, dtype=np.uint64)
        if n:
            self.ctx.check(self.ctx.lib.nts_mx_download(self.ctx.h, self.h, h1.ctypes.data, rec.ctypes.data,
                                                        pos.ctypes.data), "nts_mx_download")
        return h1, rec, pos

    @classmethod
    def from_numpy(cls, ctx, h1, rec, pos):
        h1 = np.ascontiguousarray(h1, dtype=np.uint64)
        rec = np.ascontiguousarray(rec, dtype=np.uint32)
        pos = np.ascontiguousarray(pos, dtype=np.uint64)
        h = c_vp()
        ctx.check(ctx.lib.nts_mx_upload(ctx.h, h1.ctypes.data, rec.ctypes.data, pos.ctypes.data, h1.size,
                                        ctypes.byref(h)), "nts_mx_upload")
        return cls(ctx, h)

    def kmers(self, genome, k):
        "k-mer text of every minimizer (uint8 array of len(self) * k upper-case bytes) gathered from the resident genome"
        out = np.empty(len(self) * int(k), dtype=np.uint8)
        if len(self):
            self.ctx.check(self.ctx.lib.nts_mx_kmers(self.ctx.h, genome.h, self.h, int(k), out.ctypes.data), "nts_mx_kmers")
        return out

    def screened(self, genome, k, filter_out):
        """ntJoin's read_minimizers(file, repeat_bf) (stage 3's `--filter Filter`): a new list without the minimizers whose k-mer -- the
        k bases of `genome` at their record and position -- the filter holds (nts_mx_screen)"""
        h = c_vp()
        self.ctx.check(self.ctx.lib.nts_mx_screen(self.ctx.h, genome.h, self.h, int(k), filter_out.h, ctypes.byref(h)), "nts_mx_screen")
        return Minimizers(self.ctx, h)

    def split(self, rec_base):
        """The list of a Genome.concat() batch taken apart on the device (nts_mx_split): one Minimizers per part, record ids
        local to the part; rec_base = Genome.rec_base of the batch."""
        n = len(rec_base) - 1
        base = (ctypes.c_uint32 * (n + 1))(*[int(x) for x in rec_base])
        out = (c_vp * n)()
        self.ctx.check(self.ctx.lib.nts_mx_split(self.ctx.h, self.h, n, base, out), "nts_mx_split")
        return [Minimizers(self.ctx, c_vp(out[p])) for p in range(n)]

    @classmethod
    def concat(cls, ctx, parts, rec_offsets):
        "the lists of a genome's shards, in record order, as the genome's list: part p's record numbers raised by rec_offsets[p] (nts_mx_concat)"
        n = len(parts)
        arr = (c_vp * n)(*[m.h for m in parts])
        off = (ctypes.c_uint32 * n)(*[int(x) for x in rec_offsets])
        h = c_vp()
        ctx.check(ctx.lib.nts_mx_concat(ctx.h, n, arr, off, ctypes.byref(h)), "nts_mx_concat")
        return cls(ctx, h)

    def device_ptrs(self):
        a, b, c = c_vp(), c_vp(), c_vp()
        self.ctx.lib.nts_mx_device_ptrs(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        return a.value, b.value, c.value

    def free(self):
        if self.h:
            self.ctx.lib.nts_mx_free(self.ctx.h, self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def sketch(ctx, genome, k, w, bf=None, masks=None, repeat=None):
    """`indexlr -k k -w w --long --pos [-s bf] [-r repeat]` on the resident genome.  masks: iterable of
    (record index, start, end) hard-mask intervals applied on the fly (refinement rounds).  repeat: filter-out
    Bloom filter (the reference's experimental repeat filter; served by the every-k-mer-probed kernels)."""
    n_mask, arr = 0, None
    if masks is not None and len(masks):
        n_mask = len(masks)
        if isinstance(masks, np.ndarray) and masks.dtype.itemsize == ctypes.sizeof(Interval) and masks.dtype.names:
            masks = np.ascontiguousarray(masks)                 # already in nts_interval's layout (synteny_device.INTERVAL_DTYPE)
            arr = ctypes.cast(masks.ctypes.data, ctypes.POINTER(Interval))
        else:
            arr = (Interval * n_mask)()
            for i, (r, s, e) in enumerate(masks):
                arr[i].rec, arr[i].start, arr[i].end = int(r), int(s), int(e)
    h = c_vp()
    if repeat is not None:
        ctx.check(ctx.lib.nts_sketch_ex(ctx.h, genome.h, int(k), int(w), bf.h if bf is not None else None, repeat.h,
                                        arr, n_mask, ctypes.byref(h)), "nts_sketch_ex")
    else:
        ctx.check(ctx.lib.nts_sketch(ctx.h, genome.h, int(k), int(w), bf.h if bf is not None else None,
                                     arr, n_mask, ctypes.byref(h)), "nts_sketch")
    return Minimizers(ctx, h)


class SketchPool:
    """Sketches of several resident genomes at once: every genome on a context (stream, workspaces) of its own, driven from a host
    thread of its own -- the GPU overlaps one genome's latency-bound kernels (list compaction, window decisions, gather,
    finalize, the uncovered ranges: a third of a sketch) with another's rolling.  Three 3 Gbp genomes: 5.8 ms against 6.5 one after
    the other (scripts/concurrent_sketch.py).  Same lists as sketch() per genome, in the order given; the lists belong to the
    pool's contexts (free them before close()).  The library serialises what the genomes share (the filter's summary)."""

    def __init__(self, ctx, n):
        self.main = ctx
        self.ctxs = [ctx] + [Context(ctx.device, ctx.variant) for _ in range(max(0, int(n) - 1))]
        self._pool = None

    def configure(self, fn):
        "apply fn(ctx) to every context of the pool (sketch_mode, profile, ...)"
        for c in self.ctxs:
            fn(c)

    def sketch(self, genomes, k, w, bf=None, masks=None, repeat=None):
        n = len(genomes)
        if n <= 1 or len(self.ctxs) == 1:
            return [sketch(self.main, g, k, w, bf, masks[i] if masks else None, repeat=repeat) for i, g in enumerate(genomes)]
        from concurrent.futures import ThreadPoolExecutor
        if self._pool is None:
            self._pool = ThreadPoolExecutor(max_workers=len(self.ctxs))
        out = [None] * n
        lanes = min(n, len(self.ctxs))

        def lane(c):
            for i in range(c, n, lanes):                  # (the C calls release the GIL)
                out[i] = sketch(self.ctxs[c], genomes[i], k, w, bf, masks[i] if masks else None, repeat=repeat)
        for f in [self._pool.submit(lane, c) for c in range(lanes)]:
            f.result()
        for mx in out:            # the lanes are done: the lists belong to the caller's context from here on (they outlive the pool)
            mx.ctx = self.main
        return out

    def timing(self, name):
        "(ms, launches) summed over the pool's contexts"
        ms = n = 0
        for c in self.ctxs:
            a, b = c.timing(name)
            ms, n = ms + a, n + b
        return ms, n

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
        for c in self.ctxs[1:]:
            c.close()
        self.ctxs = self.ctxs[:1]


def wrap_bloom(ctx, tensor, nbytes, k):
    """BloomFilter view over a caller-owned device buffer (a torch uint8 tensor of at least
    ceil16(nbytes) bytes, zero-initialised): lets RCCL collectives run on the very same memory."""
    bf = BloomFilter.__new__(BloomFilter)
    bf.ctx, bf.k, bf.bytes = ctx, k, int(nbytes)
    h = c_vp()
    ctx.check(ctx.lib.nts_bf_wrap(ctx.h, ctypes.c_void_p(tensor.data_ptr()), int(nbytes), ctypes.byref(h)), "nts_bf_wrap")
    bf.h = h
    bf._keepalive = tensor
    return bf


def and_raw(ctx, acc_ptr, other_ptr, nbytes):
    "acc &= other on raw device pointers (local step of the AND all-reduce)"
    ctx.check(ctx.lib.nts_and_raw(ctx.h, ctypes.c_void_p(acc_ptr), ctypes.c_void_p(other_ptr), int(nbytes)), "nts_and_raw")


def export_minimizers(ctx, mx, h1_ptr, rec_ptr, pos_ptr, wait=True):
    "device-to-device copy of a list into caller buffers; wait=False: queued only, ctx.sync() before use / mx.free()"
    fn = ctx.lib.nts_mx_export if wait else ctx.lib.nts_mx_export_async
    ctx.check(fn(ctx.h, mx.h, ctypes.c_void_p(h1_ptr), ctypes.c_void_p(rec_ptr), ctypes.c_void_p(pos_ptr)), "nts_mx_export")

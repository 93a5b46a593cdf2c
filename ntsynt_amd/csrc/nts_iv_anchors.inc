// ---- the anchors of pairs of intervals of TWO lists, and the segments between consecutive anchors (nts_iv_anchor_segments; ----
// ntsynt_amd/assess.py block_identity).  docs/design/04_16_block_identity.md.  List A and list B are one genome's records {h0, iv, off}
// each, as nts_sample_intervals returns them; mate[iv_a] names the interval of B that interval iv_a of A is paired with.  An anchor is
// a hash that A has once, B has once, and whose two intervals are mates.  All on the context's stream and in its workspace, no atomic,
// no launch per interval, no floating point:
//   1  the lists one behind the other (A first: an element's number tells its list), k_iva_split takes the hashes out
//   2  stable radix sort by hash (ivs_sort: the <uint64, uint64> pairs sort), the element's number as the value
//   3  k_iva_mark: the head of a run of exactly two records, the first of A and the second of B, whose intervals are mates writes
//      {iv_a << 32 | x, y}, x = off_a, y = off_b or, flipped, len_b - k - off_b; every other lane writes IVA_NONE
//   4  rocprim::select keeps the anchors
//   5  one stable radix sort by iv_a << 32 | x: (iv_a, x) order (x is strictly increasing within an interval: one record per offset)
//   6  k_iva_segments: one lane per anchor writes the segment behind it where the next anchor has the same iv_a, IVA_NO_KIND otherwise;
//      rocprim::select keeps the segments, in (iv_a, x) order
//   7  rocprim::run_length_encode over iv_a gives the anchors per interval, k_iva_counts stores them

constexpr uint64_t IVA_NONE = ~0ULL;          // (no anchor has it: iv_a < 2^32 - 1 is checked, so the upper half is never all ones)
constexpr uint32_t IVA_NO_KIND = 0xFFFFFFFFu; // an anchor that is the last of its interval
constexpr uint32_t IVA_NO_MATE = 0xFFFFFFFFu;
static_assert(sizeof(nts_iv_segment) == 24, "the C ABI's layout");

struct IvaAnchor
{
  uint64_t key, y; // iv_a << 32 | x; y in the oriented frame
};

struct IvaIsAnchor
{
  __host__ __device__ bool operator()(const IvaAnchor& a) const { return a.key != IVA_NONE; }
};

struct IvaIsSegment
{
  __host__ __device__ bool operator()(const nts_iv_segment& s) const { return s.kind != IVA_NO_KIND; }
};

struct IvaHigh32 // the interval of an iv_a << 32 | x word
{
  __host__ __device__ uint32_t operator()(uint64_t v) const { return (uint32_t)(v >> 32); }
};

__global__ __launch_bounds__(256) void k_iva_split(const nts_sample* __restrict__ rec, uint64_t n, uint64_t* __restrict__ h, uint64_t* __restrict__ e)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  h[i] = rec[i].h0;
  e[i] = i;
}

// records sorted by hash, A's before B's within a run
__global__ __launch_bounds__(256) void k_iva_mark(const uint64_t* __restrict__ h_sorted, const uint64_t* __restrict__ e_sorted,
                                                  const nts_sample* __restrict__ rec, uint64_t n, uint64_t n_a, const uint32_t* __restrict__ mate,
                                                  const uint32_t* __restrict__ len_b, const uint8_t* __restrict__ flip, uint64_t n_iv_a, uint32_t k,
                                                  IvaAnchor* __restrict__ out)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  IvaAnchor a{ IVA_NONE, 0 };
  const uint64_t hv = h_sorted[i];
  if ((i == 0 || h_sorted[i - 1] != hv) && i + 1 < n && h_sorted[i + 1] == hv && (i + 2 >= n || h_sorted[i + 2] != hv)) {
    const uint64_t e0 = e_sorted[i], e1 = e_sorted[i + 1];
    if (e0 < n_a && e1 >= n_a && e1 < n) {
      const nts_sample ra = rec[e0], rb = rec[e1];
      if (ra.iv < n_iv_a && mate[ra.iv] == rb.iv) {
        const uint32_t lb = len_b[ra.iv];
        const bool f = flip[ra.iv] != 0;
        if (!f || (uint64_t)rb.off + k <= lb) // (a k-mer of b lies inside b: anything else is not b's record)
          a = { ((uint64_t)ra.iv << 32) | ra.off, f ? lb - k - rb.off : rb.off };
      }
    }
  }
  out[i] = a;
}

__global__ __launch_bounds__(256) void k_iva_unzip(const IvaAnchor* __restrict__ a, uint64_t n, uint64_t* __restrict__ key, uint64_t* __restrict__ y)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  key[i] = a[i].key;
  y[i] = a[i].y;
}

// anchors in (iv_a, x) order
__global__ __launch_bounds__(256) void k_iva_segments(const uint64_t* __restrict__ key, const uint64_t* __restrict__ y, uint64_t n, uint32_t band,
                                                      uint32_t max_len, nts_iv_segment* __restrict__ out)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t w = key[i];
  nts_iv_segment s{ (uint32_t)(w >> 32), (uint32_t)w, 0u, (uint32_t)y[i], 0, IVA_NO_KIND };
  if (i + 1 < n && (key[i + 1] >> 32) == (w >> 32)) {
    const int64_t dx = (int64_t)(uint32_t)key[i + 1] - (int64_t)(uint32_t)w, dy = (int64_t)y[i + 1] - (int64_t)y[i];
    const int64_t delta = dy - dx;
    s.dx = (uint32_t)dx;
    s.dy = (int32_t)dy;
    s.kind = dy <= 0                                     ? NTS_SEG_BACKWARD
             : (dx > (int64_t)max_len || dy > (int64_t)max_len) ? NTS_SEG_LONG
             : (delta > (int64_t)band || -delta > (int64_t)band) ? NTS_SEG_OFFBAND
                                                         : NTS_SEG_CANDIDATE;
  }
  out[i] = s;
}

__global__ __launch_bounds__(256) void k_iva_counts(const uint32_t* __restrict__ iv, const uint32_t* __restrict__ cnt, const uint64_t* __restrict__ n_runs,
                                                    uint64_t cap, uint64_t n_iv, uint32_t* __restrict__ out)
{
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cap || j >= *n_runs) return;
  const uint32_t i = iv[j];
  if (i < n_iv) out[i] = cnt[j];
}

int iv_anchor_segments_run(nts_ctx* ctx, const nts_sample* recs_a, uint64_t n_a, const nts_sample* recs_b, uint64_t n_b, const uint32_t* mate,
                           uint64_t n_iv_a, const uint32_t* len_b, const uint8_t* flip, uint32_t k, uint32_t band, uint32_t max_len,
                           nts_iv_segment** segs, uint64_t* n_segs, uint32_t* anchors_per_iv)
{
  const uint64_t n = n_a + n_b;
  if (n_a > 0xFFFFFFFFull || n_b > 0xFFFFFFFFull || n > 0xFFFFFFFFull || n_iv_a >= 0xFFFFFFFFull)
    return fail(ctx, NTS_ERANGE, "nts_iv_anchor_segments: 2^32 records or more, or 2^32 - 1 intervals or more (raise the rate)");
  if (int rc = ivp_check(ctx, "nts_iv_anchor_segments", recs_a, n_a, n_iv_a)) return rc;
  if (int rc = ivp_check(ctx, "nts_iv_anchor_segments", recs_b, n_b, 0xFFFFFFFFull)) return rc; // (b's intervals are named by mate alone)
  for (uint64_t i = 0; i < n_iv_a; ++i)
    if (flip[i] > 1) return fail(ctx, NTS_EINVAL, "nts_iv_anchor_segments: flip is 0 or 1");
  if (n_iv_a) memset(anchors_per_iv, 0, n_iv_a * 4);
  if (n_a == 0 || n_b == 0 || n_iv_a == 0) return NTS_OK;
  const uint64_t cap = std::min(n_a, n_b); // (an anchor takes one record of each list)
  NTS_WS(d_rec, nts_sample*, "iva_rec", n * sizeof(nts_sample));
  NTS_WS(d_h, uint64_t*, "iva_h", n * 8);
  NTS_WS(d_e, uint64_t*, "iva_e", n * 8);
  NTS_WS(d_h2, uint64_t*, "iva_h2", n * 8);
  NTS_WS(d_e2, uint64_t*, "iva_e2", n * 8);
  NTS_WS(d_all, IvaAnchor*, "iva_all", n * sizeof(IvaAnchor));
  NTS_WS(d_anch, IvaAnchor*, "iva_anch", cap * sizeof(IvaAnchor));
  NTS_WS(d_mate, uint32_t*, "iva_mate", n_iv_a * 4);
  NTS_WS(d_lenb, uint32_t*, "iva_lenb", n_iv_a * 4);
  NTS_WS(d_flip, uint8_t*, "iva_flip", n_iv_a);
  NTS_WS(d_per, uint32_t*, "iva_per", n_iv_a * 4);
  NTS_WS(d_num, uint64_t*, "iva_num", 16);
  HIP_TRY(ctx, hipMemcpyAsync(d_rec, recs_a, n_a * sizeof(nts_sample), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_rec + n_a, recs_b, n_b * sizeof(nts_sample), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_mate, mate, n_iv_a * 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_lenb, len_b, n_iv_a * 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_flip, flip, n_iv_a, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(d_per, 0, n_iv_a * 4, ctx->stream));
  uint64_t na = 0;
  {
    ScopedTimer t(ctx, "iv_anchors_join");
    NTS_LAUNCH(k_iva_split, IVL_GRID(n), (const nts_sample*)d_rec, n, d_h, d_e);
    if (int rc = ivs_sort(ctx, d_h, d_h2, d_e, d_e2, n, 64)) return rc;
    NTS_LAUNCH(k_iva_mark, IVL_GRID(n), (const uint64_t*)d_h2, (const uint64_t*)d_e2, (const nts_sample*)d_rec, n, n_a, (const uint32_t*)d_mate,
               (const uint32_t*)d_lenb, (const uint8_t*)d_flip, n_iv_a, k, d_all);
    size_t tmp = 0;
    HIP_TRY(ctx, rocprim::select(nullptr, tmp, d_all, d_anch, d_num, n, IvaIsAnchor(), ctx->stream));
    NTS_WS(d_tmp, void*, "ivs_tmp", std::max<size_t>(tmp, 16));
    HIP_TRY(ctx, rocprim::select(d_tmp, tmp, d_all, d_anch, d_num, n, IvaIsAnchor(), ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&na, d_num, 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // (the caller's arrays are the caller's again from here)
  if (na > cap) return fail(ctx, NTS_EHIP, "nts_iv_anchor_segments: the selection returned an impossible count");
  if (na == 0) return NTS_OK;
  // (d_h, d_e, d_h2, d_e2 are free again: the anchors' keys and y, unsorted and sorted; d_all: the segments of all anchors)
  nts_iv_segment* const d_seg_all = (nts_iv_segment*)d_all;
  static_assert(sizeof(nts_iv_segment) <= 2 * sizeof(IvaAnchor), "the segments of `na` anchors fit where the marks of n >= 2 na records were");
  NTS_WS(d_seg, nts_iv_segment*, "iva_seg", na * sizeof(nts_iv_segment));
  NTS_WS(d_uiv, uint32_t*, "iva_uiv", na * 4);
  NTS_WS(d_cnt, uint32_t*, "iva_cnt", na * 4);
  uint64_t num[2] = { 0, 0 };
  {
    ScopedTimer t(ctx, "iv_anchors_segments");
    NTS_LAUNCH(k_iva_unzip, IVL_GRID(na), (const IvaAnchor*)d_anch, na, d_h, d_e);
    if (int rc = ivs_sort(ctx, d_h, d_h2, d_e, d_e2, na, 64)) return rc;
    NTS_LAUNCH(k_iva_segments, IVL_GRID(na), (const uint64_t*)d_h2, (const uint64_t*)d_e2, na, band, max_len, d_seg_all);
    size_t tmp = 0;
    HIP_TRY(ctx, rocprim::select(nullptr, tmp, d_seg_all, d_seg, d_num, na, IvaIsSegment(), ctx->stream));
    {
      NTS_WS(d_tmp, void*, "ivs_tmp", std::max<size_t>(tmp, 16));
      HIP_TRY(ctx, rocprim::select(d_tmp, tmp, d_seg_all, d_seg, d_num, na, IvaIsSegment(), ctx->stream));
    }
    auto ivs = rocprim::make_transform_iterator((const uint64_t*)d_h2, IvaHigh32());
    tmp = 0;
    HIP_TRY(ctx, rocprim::run_length_encode(nullptr, tmp, ivs, na, d_uiv, d_cnt, d_num + 1, ctx->stream));
    NTS_WS(d_tmp, void*, "ivs_tmp", std::max<size_t>(tmp, 16));
    HIP_TRY(ctx, rocprim::run_length_encode(d_tmp, tmp, ivs, na, d_uiv, d_cnt, d_num + 1, ctx->stream));
    NTS_LAUNCH(k_iva_counts, IVL_GRID(na), (const uint32_t*)d_uiv, (const uint32_t*)d_cnt, (const uint64_t*)(d_num + 1), na, n_iv_a, d_per);
    HIP_TRY(ctx, hipMemcpyAsync(num, d_num, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(anchors_per_iv, d_per, n_iv_a * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (num[0] >= na || num[1] == 0 || num[1] > na || num[0] + num[1] != na)
    return fail(ctx, NTS_EHIP, "nts_iv_anchor_segments: segments and intervals do not add up to the anchors");
  if (num[0] == 0) return NTS_OK;
  if (int rc = ivf_to_host(ctx, "nts_iv_anchor_segments", (const nts_iv_segment*)d_seg, num[0], segs)) return rc;
  *n_segs = num[0];
  return NTS_OK;
}

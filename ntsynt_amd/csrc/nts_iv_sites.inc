// ---- the sampled k-mers of several lists of gaps joined by hash against ONE genome's occurrences, grouped into sites (nts_iv_sites; ----
// ntsynt_amd/gaps.py copy_sites).  docs/design/04_13_gap_copy_sites.md.  nts_iv_links (nts_iv_links.inc) uses a hash once per list: right
// for chaining, wrong for locating the copies of a duplication.  Here multiplicity is allowed on both sides: a pair is a query record q
// (a gap's sampled k-mer) and a target record o ({h0, iv = record, off = position}) of one hash; for one gap the pairs ordered by
// (o.rec, o.pos, q's place in its list) fall into sites: maximal runs of one record whose consecutive positions differ by at most `step`.
// All on the context's stream and in its workspace, no atomic, no launch per gap:
//   1  the lists one behind the other, a gap's global id = its list's base + iv (IvlLists, the bases from the host, as nts_iv_links)
//   2  the target's hashes sorted (stable radix sort, the <uint64, uint64> pairs sort), carrying the record's index
//   3  k_ivs_count: one lane per query record, lower and upper bound of its hash in the sorted hashes = where its matches start and how
//      many there are; exclusive scan of the counts
//   4  k_ivs_pairs: ONE LANE PER OUTPUT PAIR: an upper-bound search of the lane's number in the scan finds its query record (the LAST
//      record whose scan value is <= the number: records without a match share their successor's scan value and are passed over), the
//      remainder its match; it stores the locus key rec << 32 | pos and q.off << 32 | gap id, two coalesced 8-byte stores; pairs come
//      out in query order, a query's matches in the target's order
//   5  stable sort by locus key carrying off | gap, then stable sort by the gap id (the LOWER 32 bits of off | gap: bits 0..32 of the
//      key, as nts_iv_links sorts its offsets) carrying the locus: ties stay in query order.  The gap id does not sit in the upper half:
//      a radix sort of bits 32..64 goes, from 1 025 elements on, through rocprim's merge of sorted blocks, whose comparison mask is built
//      with a shift by begin_bit + bits = 64 and then selects the lower half of the key
//   6  k_ivs_flags: head flag where the gap or the record changes or the position jumps by more than step; rise / fall of q.off against
//      the previous pair of the same site; the four extrema -- one IvsAgg per pair; inclusive scan of the head flags = the site id
//   7  one rocprim::reduce_by_key over the site id; k_ivs_sites turns gap ids back into (list, iv); rocprim::select keeps the sites with
//      hits >= min_hits, in (list_q, iv_q, rec_t, first_t) order

struct IvsAgg
{
  uint32_t gap, rec, hits, fwd, rev, min_q, max_q, first_t, last_t;
};

struct IvsAdd // (gap and rec are equal within a site)
{
  __host__ __device__ IvsAgg operator()(const IvsAgg& x, const IvsAgg& y) const
  {
    return { x.gap, x.rec, x.hits + y.hits, x.fwd + y.fwd, x.rev + y.rev, x.min_q < y.min_q ? x.min_q : y.min_q, x.max_q > y.max_q ? x.max_q : y.max_q,
             x.first_t < y.first_t ? x.first_t : y.first_t, x.last_t > y.last_t ? x.last_t : y.last_t };
  }
};

struct IvsKeep
{
  uint32_t min_hits;
  __host__ __device__ bool operator()(const nts_iv_site& s) const { return s.hits >= min_hits; }
};
static_assert(sizeof(nts_iv_site) == 40, "the C ABI's layout");

__global__ __launch_bounds__(256) void k_ivs_split(const nts_sample* __restrict__ target, uint64_t nt, uint64_t* __restrict__ h, uint64_t* __restrict__ e)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nt) return;
  h[i] = target[i].h0;
  e[i] = i;
}

// lo[q] = the first place of q's hash in the sorted target hashes, cnt[q] = how many places hold it
__global__ __launch_bounds__(256) void k_ivs_count(const nts_sample* __restrict__ rec, uint64_t n, const uint64_t* __restrict__ th, uint64_t nt,
                                                   uint32_t* __restrict__ lo, uint32_t* __restrict__ cnt)
{
  const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  const uint64_t h = rec[q].h0;
  uint64_t a = 0, b = nt;
  while (a < b) { // lower bound: the first place with th >= h
    const uint64_t m = (a + b) >> 1;
    if (th[m] < h)
      a = m + 1;
    else
      b = m;
  }
  const uint64_t first = a;
  b = nt;
  while (a < b) { // upper bound: the first place with th > h
    const uint64_t m = (a + b) >> 1;
    if (th[m] <= h)
      a = m + 1;
    else
      b = m;
  }
  lo[q] = (uint32_t)first;
  cnt[q] = (uint32_t)(a - first);
}

__global__ __launch_bounds__(256) void k_ivs_pairs(const uint64_t* __restrict__ at, uint64_t n, uint64_t n_pairs, const nts_sample* __restrict__ rec,
                                                   const uint32_t* __restrict__ lo, const uint64_t* __restrict__ te, const nts_sample* __restrict__ target,
                                                   uint64_t nt, IvlLists L, uint64_t* __restrict__ locus, uint64_t* __restrict__ gq)
{
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  uint64_t a = 0, b = n;
  while (a < b) { // upper bound: the first record whose pairs start behind p (at[0] = 0 <= p: a >= 1)
    const uint64_t m = (a + b) >> 1;
    if (at[m] <= p)
      a = m + 1;
    else
      b = m;
  }
  const uint64_t q = a - 1;
  const uint64_t place = (uint64_t)lo[q] + (p - at[q]);
  if (place >= nt) return; // (cannot happen: the scan's own counts)
  const uint64_t t = te[place];
  if (t >= nt) return;
  const nts_sample o = target[t], r = rec[q];
  locus[p] = ((uint64_t)o.iv << 32) | o.off;
  gq[p] = ((uint64_t)r.off << 32) | (uint64_t)(L.base[ivl_list_of_elem(L, q)] + r.iv);
}

// pairs in (gap, rec, pos, query) order
__global__ __launch_bounds__(256) void k_ivs_flags(const uint64_t* __restrict__ gq, const uint64_t* __restrict__ locus, uint64_t n, uint32_t step,
                                                   uint32_t* __restrict__ head, IvsAgg* __restrict__ agg)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t g = gq[i], l = locus[i];
  const uint32_t gap = (uint32_t)g, off = (uint32_t)(g >> 32), rec = (uint32_t)(l >> 32), pos = (uint32_t)l;
  bool first = i == 0;
  uint32_t fwd = 0, rev = 0;
  if (!first) {
    const uint64_t pg = gq[i - 1], pl = locus[i - 1];
    first = (uint32_t)pg != gap || (uint32_t)(pl >> 32) != rec || pos - (uint32_t)pl > step; // (sorted: pos >= the previous one's)
    if (!first) {
      fwd = off > (uint32_t)(pg >> 32) ? 1u : 0u;
      rev = off < (uint32_t)(pg >> 32) ? 1u : 0u;
    }
  }
  head[i] = first ? 1u : 0u;
  agg[i] = { gap, rec, 1u, fwd, rev, off, off, pos, pos };
}

__global__ __launch_bounds__(256) void k_ivs_sites(const IvsAgg* __restrict__ agg, uint64_t n, IvlLists L, nts_iv_site* __restrict__ out)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const IvsAgg g = agg[i];
  uint32_t l = 0;
  while (l + 1 < L.n && L.base[l + 1] <= g.gap) ++l; // (a list without a gap has its successor's base: the last of them is the one)
  out[i] = { l, g.gap - L.base[l], g.rec, g.hits, g.fwd, g.rev, g.min_q, g.max_q, g.first_t, g.last_t };
}

int ivs_sort(nts_ctx* ctx, const uint64_t* keys, uint64_t* keys_out, const uint64_t* vals, uint64_t* vals_out, uint64_t n, unsigned end_bit)
{
  size_t tmp = 0;
  HIP_TRY(ctx, rocprim::radix_sort_pairs(nullptr, tmp, keys, keys_out, vals, vals_out, n, 0, end_bit, ctx->stream));
  NTS_WS(d_tmp, void*, "ivs_tmp", std::max<size_t>(tmp, 16));
  HIP_TRY(ctx, rocprim::radix_sort_pairs(d_tmp, tmp, keys, keys_out, vals, vals_out, n, 0, end_bit, ctx->stream));
  return NTS_OK;
}

int iv_sites_run(nts_ctx* ctx, uint32_t n_lists, const nts_sample* const* lists, const uint64_t* n_in, const nts_sample* target, uint64_t nt,
                 uint32_t step, uint32_t min_hits, nts_iv_site** out, uint64_t* n_out)
{
  IvlLists L;
  memset(&L, 0, sizeof(L));
  L.n = n_lists;
  uint64_t n = 0, n_gaps = 0;
  for (uint32_t l = 0; l < n_lists; ++l) {
    L.at[l] = n;
    L.base[l] = (uint32_t)n_gaps;
    uint32_t top = 0;
    for (uint64_t q = 0; q < n_in[l]; ++q) top = std::max(top, lists[l][q].iv);
    if (n_in[l]) n_gaps += (uint64_t)top + 1;
    n += n_in[l];
    if (n_gaps > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_iv_sites: 2^32 gaps or more over all lists");
  }
  L.at[n_lists] = n;
  L.base[n_lists] = (uint32_t)n_gaps;
  if (n > 0xFFFFFFFFull || nt > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_iv_sites: 2^32 records or more");
  if (n == 0 || nt == 0) return NTS_OK;
  // ---- 1, 2, 3: the records, the target's hashes sorted, matches per query record
  NTS_WS(d_rec, nts_sample*, "ivs_rec", n * sizeof(nts_sample));
  NTS_WS(d_tgt, nts_sample*, "ivs_tgt", nt * sizeof(nts_sample));
  NTS_WS(d_th, uint64_t*, "ivs_th", nt * 8);
  NTS_WS(d_te, uint64_t*, "ivs_te", nt * 8);
  NTS_WS(d_th2, uint64_t*, "ivs_th2", nt * 8);
  NTS_WS(d_te2, uint64_t*, "ivs_te2", nt * 8);
  NTS_WS(d_lo, uint32_t*, "ivs_lo", n * 4);
  NTS_WS(d_cnt, uint32_t*, "ivs_cnt", n * 4);
  NTS_WS(d_at, uint64_t*, "ivs_at", n * 8);
  NTS_WS(d_num, uint64_t*, "ivs_num", 8);
  for (uint32_t l = 0; l < n_lists; ++l)
    if (n_in[l]) HIP_TRY(ctx, hipMemcpyAsync(d_rec + L.at[l], lists[l], n_in[l] * sizeof(nts_sample), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_tgt, target, nt * sizeof(nts_sample), hipMemcpyHostToDevice, ctx->stream));
  {
    ScopedTimer t(ctx, "iv_sites_join");
    NTS_LAUNCH(k_ivs_split, IVL_GRID(nt), d_tgt, nt, d_th, d_te);
    if (int rc = ivs_sort(ctx, d_th, d_th2, d_te, d_te2, nt, 64)) return rc;
    NTS_LAUNCH(k_ivs_count, IVL_GRID(n), d_rec, n, d_th2, nt, d_lo, d_cnt);
    if (int rc = scan_counts(ctx, d_cnt, n, d_at)) return rc;
  }
  uint32_t last_cnt = 0;
  uint64_t last_at = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&last_cnt, d_cnt + (n - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(&last_at, d_at + (n - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // (the caller's host arrays are the caller's again from here)
  const uint64_t np = last_at + last_cnt;
  if (np > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_iv_sites: 2^32 pairs or more (lower the cap or raise the rate)");
  if (np == 0) return NTS_OK;
  // ---- 4, 5, 6, 7: the pairs, sorted by (gap, locus), flagged, reduced per site
  NTS_WS(d_locus, uint64_t*, "ivs_locus", np * 8);
  NTS_WS(d_gq, uint64_t*, "ivs_gq", np * 8);
  NTS_WS(d_locus2, uint64_t*, "ivs_locus2", np * 8);
  NTS_WS(d_gq2, uint64_t*, "ivs_gq2", np * 8);
  NTS_WS(d_head, uint32_t*, "ivs_head", np * 4);
  NTS_WS(d_sid, uint32_t*, "ivs_sid", np * 4);
  NTS_WS(d_agg, IvsAgg*, "ivs_agg", np * sizeof(IvsAgg));
  NTS_WS(d_usid, uint32_t*, "ivs_usid", np * 4);
  NTS_WS(d_uagg, IvsAgg*, "ivs_uagg", np * sizeof(IvsAgg));
  uint64_t nu = 0;
  {
    ScopedTimer t(ctx, "iv_sites_pairs");
    NTS_LAUNCH(k_ivs_pairs, IVL_GRID(np), (const uint64_t*)d_at, n, np, (const nts_sample*)d_rec, (const uint32_t*)d_lo, (const uint64_t*)d_te2,
               (const nts_sample*)d_tgt, nt, L, d_locus, d_gq);
    if (int rc = ivs_sort(ctx, d_locus, d_locus2, d_gq, d_gq2, np, 64)) return rc;
    if (int rc = ivs_sort(ctx, d_gq2, d_gq, d_locus2, d_locus, np, 32)) return rc; // (by the gap id only: within a gap the locus order stays)
    NTS_LAUNCH(k_ivs_flags, IVL_GRID(np), (const uint64_t*)d_gq, (const uint64_t*)d_locus, np, step, d_head, d_agg);
    size_t tmp = 0;
    HIP_TRY(ctx, rocprim::inclusive_scan(nullptr, tmp, d_head, d_sid, np, rocprim::plus<uint32_t>(), ctx->stream));
    {
      NTS_WS(d_tmp, void*, "ivs_tmp", std::max<size_t>(tmp, 16));
      HIP_TRY(ctx, rocprim::inclusive_scan(d_tmp, tmp, d_head, d_sid, np, rocprim::plus<uint32_t>(), ctx->stream));
    }
    tmp = 0;
    HIP_TRY(ctx, rocprim::reduce_by_key(nullptr, tmp, d_sid, d_agg, np, d_usid, d_uagg, d_num, IvsAdd(), rocprim::equal_to<uint32_t>(), ctx->stream));
    NTS_WS(d_tmp, void*, "ivs_tmp", std::max<size_t>(tmp, 16));
    HIP_TRY(ctx, rocprim::reduce_by_key(d_tmp, tmp, d_sid, d_agg, np, d_usid, d_uagg, d_num, IvsAdd(), rocprim::equal_to<uint32_t>(), ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&nu, d_num, 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (nu == 0 || nu > np) return fail(ctx, NTS_EHIP, "nts_iv_sites: the per-site reduction returned an impossible count");
  NTS_WS(d_all, nts_iv_site*, "ivs_all", nu * sizeof(nts_iv_site));
  NTS_WS(d_kept, nts_iv_site*, "ivs_kept", nu * sizeof(nts_iv_site));
  uint64_t nk = 0;
  {
    ScopedTimer t(ctx, "iv_sites_select");
    NTS_LAUNCH(k_ivs_sites, IVL_GRID(nu), (const IvsAgg*)d_uagg, nu, L, d_all);
    size_t tmp = 0;
    HIP_TRY(ctx, rocprim::select(nullptr, tmp, d_all, d_kept, d_num, nu, IvsKeep{ min_hits }, ctx->stream));
    NTS_WS(d_tmp, void*, "ivs_tmp", std::max<size_t>(tmp, 16));
    HIP_TRY(ctx, rocprim::select(d_tmp, tmp, d_all, d_kept, d_num, nu, IvsKeep{ min_hits }, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&nk, d_num, 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (nk > nu) return fail(ctx, NTS_EHIP, "nts_iv_sites: the selection returned an impossible count");
  if (nk == 0) return NTS_OK;
  nts_iv_site* host = (nts_iv_site*)malloc(nk * sizeof(nts_iv_site));
  if (!host) return fail(ctx, NTS_ENOMEM, "nts_iv_sites: host memory for the sites");
  hipError_t e = hipMemcpyAsync(host, d_kept, nk * sizeof(nts_iv_site), hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t e_sync = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess || e_sync != hipSuccess) free(host);
  HIP_TRY(ctx, e);
  HIP_TRY(ctx, e_sync);
  *out = host;
  *n_out = nk;
  return NTS_OK;
}

// ---- sampled k-mers of several lists of intervals joined by hash into links (nts_iv_links; ntsynt_amd/gaps.py links) ---------------
// docs/design/04_10_gap_links.md.  A list is one genome's records {h0, iv, off} as nts_bf_sample_intervals returns them.  A hash is
// usable when no list has it twice; an anchor of interval a (list A) and interval b (list B, A < B) is a usable hash in both; a link
// is a pair (a, b) with at least min_anchors anchors.  All on the context's stream, no atomic, no per-link launch:
//   1  the lists one behind the other (list-major: an element's number orders it by list), k_ivl_split takes hash and list out of them
//   2  stable radix sort by hash (the <uint64, uint64> pairs sort the graph build instantiates): a run of equal hashes is in list order
//   3  k_ivl_runs: the head of a run without two neighbours of one list counts its pairs, m (m - 1) / 2 for m <= n_lists members (a
//      run longer than n_lists has a list twice: no head looks further than n_lists + 1 elements); exclusive scan
//   4  k_ivl_pairs: every kept head writes its pairs: key = (global interval a) << 32 | (global interval b), off_a, off_b; an interval's
//      global number is its list's base + iv (bases: prefix sums of the lists' largest iv + 1, from the host)
//   5  stable sort by off_a, then by key: within a key the pairs are ordered by off_a, ties (no two anchors of one link share an
//      offset when the records come from one genome's sweep; hand-made lists may) by hash
//   6  k_ivl_flags: count 1, rise / fall of off_b against the next pair of the same key, the four offsets -- one IvlAgg per pair
//   7  rocprim::reduce_by_key adds them up per key (sums and extrema); k_ivl_links turns keys back into (list, iv) pairs and
//      rocprim::select keeps the links with anchors >= min_anchors, in key order = (list_a, iv_a, list_b, iv_b) order

struct IvlAgg
{
  uint32_t anchors, fwd, rev, min_a, max_a, min_b, max_b;
};

struct IvlAdd
{
  __host__ __device__ IvlAgg operator()(const IvlAgg& x, const IvlAgg& y) const
  {
    return { x.anchors + y.anchors, x.fwd + y.fwd,           x.rev + y.rev,          x.min_a < y.min_a ? x.min_a : y.min_a,
             x.max_a > y.max_a ? x.max_a : y.max_a,          x.min_b < y.min_b ? x.min_b : y.min_b, x.max_b > y.max_b ? x.max_b : y.max_b };
  }
};

struct IvlKeep
{
  uint32_t min_anchors;
  __host__ __device__ bool operator()(const nts_iv_link& l) const { return l.anchors >= min_anchors; }
};
static_assert(sizeof(nts_iv_link) == 44 && sizeof(nts_sample) == 16, "the C ABI's layouts");

constexpr uint32_t IVL_MAX_LISTS = 64; // (list_at / base tables ride in the kernel arguments)
struct IvlLists
{
  uint32_t n;
  uint64_t at[IVL_MAX_LISTS + 1];   // elements before list l
  uint32_t base[IVL_MAX_LISTS + 1]; // global number of list l's interval 0
};

__device__ __forceinline__ uint32_t ivl_list_of_elem(const IvlLists& L, uint64_t e)
{
  uint32_t l = 0;
  while (l + 1 < L.n && L.at[l + 1] <= e) ++l;
  return l;
}

__global__ __launch_bounds__(256) void k_ivl_split(const nts_sample* __restrict__ rec, uint64_t n, IvlLists L, uint64_t* __restrict__ h,
                                                   uint32_t* __restrict__ list)
{
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  h[e] = rec[e].h0;
  list[e] = ivl_list_of_elem(L, e);
}

// pairs[i] = the pairs of the run that starts at i when it is kept, else 0
__global__ __launch_bounds__(256) void k_ivl_runs(const uint64_t* __restrict__ h_sorted, const uint64_t* __restrict__ e_sorted,
                                                  const uint32_t* __restrict__ list, uint64_t n, uint32_t n_lists, uint64_t* __restrict__ pairs)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t out = 0;
  const uint64_t hv = h_sorted[i];
  if (i == 0 || h_sorted[i - 1] != hv) {
    uint32_t m = 1, prev = list[e_sorted[i]];
    bool twice = false;
    for (uint64_t j = i + 1; j < n && h_sorted[j] == hv; ++j) {
      const uint32_t l = list[e_sorted[j]];
      if (l == prev || ++m > n_lists) { // (list order within the run: a list's two are neighbours)
        twice = true;
        break;
      }
      prev = l;
    }
    if (!twice) out = (uint64_t)m * (m - 1) / 2;
  }
  pairs[i] = out;
}

__global__ __launch_bounds__(256) void k_ivl_pairs(const uint64_t* __restrict__ h_sorted, const uint64_t* __restrict__ e_sorted,
                                                   const uint32_t* __restrict__ list, const nts_sample* __restrict__ rec, uint64_t n,
                                                   const uint64_t* __restrict__ pairs, const uint64_t* __restrict__ pair_at, IvlLists L,
                                                   uint64_t n_pairs, uint64_t* __restrict__ key, uint64_t* __restrict__ off_a, uint32_t* __restrict__ off_b)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || pairs[i] == 0) return;
  const uint64_t hv = h_sorted[i];
  uint64_t p = pair_at[i];
  if (p + pairs[i] > n_pairs) return; // (cannot happen: the scan's own total)
  for (uint64_t x = i; x < n && h_sorted[x] == hv; ++x) {
    const uint64_t ex = e_sorted[x];
    const uint64_t ga = L.base[list[ex]] + rec[ex].iv;
    for (uint64_t y = x + 1; y < n && h_sorted[y] == hv; ++y) {
      const uint64_t ey = e_sorted[y];
      key[p] = (ga << 32) | (uint64_t)(L.base[list[ey]] + rec[ey].iv);
      off_a[p] = rec[ex].off;
      off_b[p] = rec[ey].off;
      ++p;
    }
  }
}

__global__ __launch_bounds__(256) void k_ivl_gather_key(const uint64_t* __restrict__ key, const uint64_t* __restrict__ perm, uint64_t n,
                                                        uint64_t* __restrict__ out)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = key[perm[i]];
}

// pairs in (key, off_a) order: perm[i] = the pair at place i
__global__ __launch_bounds__(256) void k_ivl_flags(const uint64_t* __restrict__ key_sorted, const uint64_t* __restrict__ perm,
                                                   const uint64_t* __restrict__ off_a, const uint32_t* __restrict__ off_b, uint64_t n,
                                                   IvlAgg* __restrict__ agg)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t p = perm[i];
  const uint32_t a = (uint32_t)off_a[p], b = off_b[p];
  uint32_t fwd = 0, rev = 0;
  if (i + 1 < n && key_sorted[i + 1] == key_sorted[i]) {
    const uint32_t nb = off_b[perm[i + 1]];
    fwd = nb > b ? 1u : 0u;
    rev = nb < b ? 1u : 0u;
  }
  agg[i] = { 1u, fwd, rev, a, a, b, b };
}

__global__ __launch_bounds__(256) void k_ivl_links(const uint64_t* __restrict__ key, const IvlAgg* __restrict__ agg, uint64_t n, IvlLists L,
                                                   nts_iv_link* __restrict__ out)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t ga = (uint32_t)(key[i] >> 32), gb = (uint32_t)key[i];
  uint32_t la = 0, lb = 0;
  while (la + 1 < L.n && L.base[la + 1] <= ga) ++la; // (a list without an interval has its successor's base: the last of them is the one)
  while (lb + 1 < L.n && L.base[lb + 1] <= gb) ++lb;
  const IvlAgg g = agg[i];
  out[i] = { la, ga - L.base[la], lb, gb - L.base[lb], g.anchors, g.fwd, g.rev, g.min_a, g.max_a, g.min_b, g.max_b };
}

int ivl_sort(nts_ctx* ctx, const uint64_t* keys, uint64_t* keys_out, const uint64_t* vals, uint64_t* vals_out, uint64_t n, unsigned end_bit)
{
  size_t tmp = 0;
  HIP_TRY(ctx, rocprim::radix_sort_pairs(nullptr, tmp, keys, keys_out, vals, vals_out, n, 0, end_bit, ctx->stream));
  NTS_WS(d_tmp, void*, "ivl_tmp", std::max<size_t>(tmp, 16));
  HIP_TRY(ctx, rocprim::radix_sort_pairs(d_tmp, tmp, keys, keys_out, vals, vals_out, n, 0, end_bit, ctx->stream));
  return NTS_OK;
}

__global__ __launch_bounds__(256) void k_ivl_iota(uint64_t* __restrict__ v, uint64_t n)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = i;
}

#define IVL_GRID(n) dim3((uint32_t)(((n) + 255) / 256)), dim3(256), 0, ctx->stream

int iv_links_run(nts_ctx* ctx, uint32_t n_lists, const nts_sample* const* lists, const uint64_t* n_in, uint32_t min_anchors, nts_iv_link** out,
                 uint64_t* n_out)
{
  IvlLists L;
  memset(&L, 0, sizeof(L));
  L.n = n_lists;
  uint64_t n = 0, n_iv = 0;
  for (uint32_t l = 0; l < n_lists; ++l) {
    L.at[l] = n;
    L.base[l] = (uint32_t)n_iv;
    uint32_t top = 0;
    for (uint64_t q = 0; q < n_in[l]; ++q) top = std::max(top, lists[l][q].iv);
    if (n_in[l]) n_iv += (uint64_t)top + 1;
    n += n_in[l];
    if (n_iv > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_iv_links: 2^32 intervals or more over all lists");
  }
  L.at[n_lists] = n;
  L.base[n_lists] = (uint32_t)n_iv;
  if (n > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_iv_links: 2^32 records or more");
  if (n == 0 || n_lists < 2) return NTS_OK;
  // ---- 1, 2: the records, their hashes sorted
  NTS_WS(d_rec, nts_sample*, "ivl_rec", n * sizeof(nts_sample));
  NTS_WS(d_h, uint64_t*, "ivl_h", n * 8);
  NTS_WS(d_e, uint64_t*, "ivl_e", n * 8);
  NTS_WS(d_h2, uint64_t*, "ivl_h2", n * 8);
  NTS_WS(d_e2, uint64_t*, "ivl_e2", n * 8);
  NTS_WS(d_list, uint32_t*, "ivl_list", n * 4);
  for (uint32_t l = 0; l < n_lists; ++l)
    if (n_in[l]) HIP_TRY(ctx, hipMemcpyAsync(d_rec + L.at[l], lists[l], n_in[l] * sizeof(nts_sample), hipMemcpyHostToDevice, ctx->stream));
  {
    ScopedTimer t(ctx, "iv_links_join");
    NTS_LAUNCH(k_ivl_split, IVL_GRID(n), d_rec, n, L, d_h, d_list);
    NTS_LAUNCH(k_ivl_iota, IVL_GRID(n), d_e, n);
    if (int rc = ivl_sort(ctx, d_h, d_h2, d_e, d_e2, n, 64)) return rc;
    // ---- 3: runs, pairs per run (d_h is free again: the counts; d_e: their scan)
    NTS_LAUNCH(k_ivl_runs, IVL_GRID(n), d_h2, d_e2, d_list, n, n_lists, d_h);
    if (int rc = scan_counts(ctx, d_h, n, d_e)) return rc;
  }
  uint64_t last_cnt = 0, last_at = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&last_cnt, d_h + (n - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(&last_at, d_e + (n - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // (the lists' host arrays are the caller's again from here)
  const uint64_t np = last_cnt + last_at;
  if (np > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_iv_links: 2^32 anchor pairs or more");
  if (np == 0) return NTS_OK;
  // ---- 4, 5: the pairs, sorted by (key, off_a)
  NTS_WS(d_key, uint64_t*, "ivl_key", np * 8);
  NTS_WS(d_offa, uint64_t*, "ivl_offa", np * 8);
  NTS_WS(d_offb, uint32_t*, "ivl_offb", np * 4);
  NTS_WS(d_p0, uint64_t*, "ivl_p0", np * 8);
  NTS_WS(d_p1, uint64_t*, "ivl_p1", np * 8);
  NTS_WS(d_k1, uint64_t*, "ivl_k1", np * 8);
  NTS_WS(d_k2, uint64_t*, "ivl_k2", np * 8);
  NTS_WS(d_agg, IvlAgg*, "ivl_agg", np * sizeof(IvlAgg));
  NTS_WS(d_ukey, uint64_t*, "ivl_ukey", np * 8);
  NTS_WS(d_uagg, IvlAgg*, "ivl_uagg", np * sizeof(IvlAgg));
  NTS_WS(d_cnt, uint64_t*, "ivl_cnt", 8);
  uint64_t nu = 0;
  {
    ScopedTimer t(ctx, "iv_links_pairs");
    NTS_LAUNCH(k_ivl_pairs, IVL_GRID(n), d_h2, d_e2, d_list, d_rec, n, d_h, d_e, L, np, d_key, d_offa, d_offb);
    NTS_LAUNCH(k_ivl_iota, IVL_GRID(np), d_p0, np);
    if (int rc = ivl_sort(ctx, d_offa, d_k1, d_p0, d_p1, np, 32)) return rc; // (d_k1: the sorted offsets, not used)
    NTS_LAUNCH(k_ivl_gather_key, IVL_GRID(np), d_key, d_p1, np, d_k1);
    if (int rc = ivl_sort(ctx, d_k1, d_k2, d_p1, d_p0, np, 64)) return rc;
    // ---- 6, 7: per key
    NTS_LAUNCH(k_ivl_flags, IVL_GRID(np), d_k2, d_p0, d_offa, d_offb, np, d_agg);
    size_t tmp = 0;
    HIP_TRY(ctx, rocprim::reduce_by_key(nullptr, tmp, d_k2, d_agg, np, d_ukey, d_uagg, d_cnt, IvlAdd(), rocprim::equal_to<uint64_t>(), ctx->stream));
    NTS_WS(d_tmp, void*, "ivl_tmp", std::max<size_t>(tmp, 16));
    HIP_TRY(ctx, rocprim::reduce_by_key(d_tmp, tmp, d_k2, d_agg, np, d_ukey, d_uagg, d_cnt, IvlAdd(), rocprim::equal_to<uint64_t>(), ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&nu, d_cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (nu == 0 || nu > np) return fail(ctx, NTS_EHIP, "nts_iv_links: the per-key reduction returned an impossible count");
  NTS_WS(d_all, nts_iv_link*, "ivl_all", nu * sizeof(nts_iv_link));
  NTS_WS(d_kept, nts_iv_link*, "ivl_kept", nu * sizeof(nts_iv_link));
  uint64_t nk = 0;
  {
    ScopedTimer t(ctx, "iv_links_select");
    NTS_LAUNCH(k_ivl_links, IVL_GRID(nu), d_ukey, d_uagg, nu, L, d_all);
    size_t tmp = 0;
    HIP_TRY(ctx, rocprim::select(nullptr, tmp, d_all, d_kept, d_cnt, nu, IvlKeep{ min_anchors }, ctx->stream));
    NTS_WS(d_tmp, void*, "ivl_tmp", std::max<size_t>(tmp, 16));
    HIP_TRY(ctx, rocprim::select(d_tmp, tmp, d_all, d_kept, d_cnt, nu, IvlKeep{ min_anchors }, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&nk, d_cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (nk > nu) return fail(ctx, NTS_EHIP, "nts_iv_links: the selection returned an impossible count");
  if (nk == 0) return NTS_OK;
  nts_iv_link* host = (nts_iv_link*)malloc(nk * sizeof(nts_iv_link));
  if (!host) return fail(ctx, NTS_ENOMEM, "nts_iv_links: host memory for the links");
  hipError_t e = hipMemcpyAsync(host, d_kept, nk * sizeof(nts_iv_link), hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t e_sync = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess || e_sync != hipSuccess) free(host);
  HIP_TRY(ctx, e);
  HIP_TRY(ctx, e_sync);
  *out = host;
  *n_out = nk;
  return NTS_OK;
}

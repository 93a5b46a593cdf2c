// ---- the tandem arrays grouped into families, and every family found genome-wide (nts_iv_period_hashes, nts_iv_families, ----
// nts_iv_family_sites; ntsynt_amd/gaps.py families).  docs/design/04_15_gap_families.md.  Three passes, each linear in its records: an
// array is reduced to the distinct hashes that carry its period, the arrays that share a hash are joined into families, and one genome's
// occurrences of those hashes fall into sites per family.  All on the context's stream and in its workspace, no atomic, no launch per
// interval or array, no floating point.
// nts_iv_period_hashes:
//   1 - 3  ivp_lags (nts_iv_periods.inc): the records in (iv, h0, off) order and every record's lag
//   4  k_ivf_mark: one lane per record; head flag where iv or h0 changes; the value {h0, iv, 1 when the lag is period[iv], else 0}
//   5  inclusive scan of the head flags = the run id; one rocprim::reduce_by_key adds the values per run; rocprim::select keeps the
//      runs with a count: (iv, h0) order, off = the count
// nts_iv_families:
//   1  k_ivf_split: h0 and iv (64-bit words) per pair; stable radix sort by iv carrying h0, then by h0 carrying iv: (h0, iv) order
//   2  k_ivf_edges: one lane per pair; a pair whose predecessor has the same h0 and another iv (a smaller one: the order) gives the edge
//      predecessor's iv << 32 | iv, any other IVF_NONE (no edge equals it: its two halves would be equal)
//   3  radix sort of the edges, rocprim::run_length_encode = the distinct edges, the run of IVF_NONE last (lane 0 has no predecessor:
//      there is one); run_length_encode of the sorted h0 = the distinct hashes and how many pairs hold each; a scan of those counts
//      and k_ivf_first give the iv of each hash's first pair
//   4  host: union-find over the edges, the smaller root wins; family[a] = a's root; hash_family[j] = the root of the first pair's iv
// nts_iv_family_sites:
//   1  k_ivf_lookup: one lane per occurrence; binary search of its h0 in the ascending hashes; the key = the family, or 2^32 for a
//      hash that is no member (it sorts behind every family and counts no hit); the value rec << 32 | off
//   2  one stable radix sort on the key (33 bits): the input order supplies (rec, off) within a family
//   3  k_ivf_breaks: head flag where the family or the record changes or off jumps by more than step; {family, rec, off, off, 1}
//   4  inclusive scan = the site id; one rocprim::reduce_by_key; rocprim::select keeps hits >= min_hits: (family, rec, first) order

constexpr uint64_t IVF_NONE = ~0ULL;
constexpr uint64_t IVF_NO_FAMILY = 1ULL << 32;
static_assert(sizeof(nts_iv_fsite) == 20, "the C ABI's layout");
static_assert(sizeof(nts_sample) == 16, "the C ABI's layout");

struct IvfCount // (h0 and iv are equal within a run)
{
  __host__ __device__ nts_sample operator()(const nts_sample& x, const nts_sample& y) const { return { x.h0, x.iv, x.off + y.off }; }
};

struct IvfHas
{
  __host__ __device__ bool operator()(const nts_sample& s) const { return s.off > 0; }
};

struct IvfAdd // (family and rec are equal within a site)
{
  __host__ __device__ nts_iv_fsite operator()(const nts_iv_fsite& x, const nts_iv_fsite& y) const
  {
    return { x.family, x.rec, x.first < y.first ? x.first : y.first, x.last > y.last ? x.last : y.last, x.hits + y.hits };
  }
};

struct IvfKeep
{
  uint32_t min_hits;
  __host__ __device__ bool operator()(const nts_iv_fsite& s) const { return s.hits >= min_hits; }
};

// records in (iv, h0, off) order with their lags
__global__ __launch_bounds__(256) void k_ivf_mark(const uint64_t* __restrict__ h, const uint64_t* __restrict__ v, const uint32_t* __restrict__ lag, uint64_t n,
                                                  const uint32_t* __restrict__ period, uint64_t n_iv, uint32_t* __restrict__ head, nts_sample* __restrict__ val)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t hi = h[i];
  const uint32_t iv = (uint32_t)v[i], d = lag[i];
  const uint32_t p = iv < n_iv ? period[iv] : 0u;
  head[i] = (i == 0 || (uint32_t)v[i - 1] != iv || h[i - 1] != hi) ? 1u : 0u;
  val[i] = { hi, iv, (p && d == p) ? 1u : 0u };
}

__global__ __launch_bounds__(256) void k_ivf_split(const nts_sample* __restrict__ pair, uint64_t n, uint64_t* __restrict__ h, uint64_t* __restrict__ a)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const nts_sample r = pair[i];
  h[i] = r.h0;
  a[i] = r.iv;
}

// pairs in (h0, iv) order
__global__ __launch_bounds__(256) void k_ivf_edges(const uint64_t* __restrict__ h, const uint64_t* __restrict__ a, uint64_t n, uint64_t* __restrict__ edge)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t e = IVF_NONE;
  if (i > 0 && h[i - 1] == h[i] && a[i - 1] != a[i]) e = (a[i - 1] << 32) | a[i];
  edge[i] = e;
}

// hash j's first pair stands at at[j] of the sorted pairs
__global__ __launch_bounds__(256) void k_ivf_first(const uint64_t* __restrict__ a, uint64_t n, const uint64_t* __restrict__ at, uint64_t nh,
                                                   uint32_t* __restrict__ first)
{
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nh) return;
  const uint64_t p = at[j];
  first[j] = p < n ? (uint32_t)a[p] : 0xFFFFFFFFu; // (cannot happen: the scan's own counts; the host refuses the value)
}

__global__ __launch_bounds__(256) void k_ivf_lookup(const nts_sample* __restrict__ occ, uint64_t n, const uint64_t* __restrict__ hashes,
                                                    const uint32_t* __restrict__ hash_family, uint64_t nh, uint64_t* __restrict__ key, uint64_t* __restrict__ val)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const nts_sample o = occ[i];
  uint64_t a = 0, b = nh;
  while (a < b) { // lower bound: the first place with hashes >= h0
    const uint64_t m = (a + b) >> 1;
    if (hashes[m] < o.h0)
      a = m + 1;
    else
      b = m;
  }
  key[i] = (a < nh && hashes[a] == o.h0) ? (uint64_t)hash_family[a] : IVF_NO_FAMILY;
  val[i] = ((uint64_t)o.iv << 32) | o.off;
}

// occurrences in (family, rec, off) order, those of no family last
__global__ __launch_bounds__(256) void k_ivf_breaks(const uint64_t* __restrict__ key, const uint64_t* __restrict__ val, uint64_t n, uint32_t step,
                                                    uint32_t* __restrict__ head, nts_iv_fsite* __restrict__ agg)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t f = key[i], w = val[i];
  const uint32_t rec = (uint32_t)(w >> 32), off = (uint32_t)w;
  bool first = i == 0;
  if (!first) {
    const uint64_t pw = val[i - 1];
    first = key[i - 1] != f || (uint32_t)(pw >> 32) != rec || off - (uint32_t)pw > step; // (sorted: off >= the previous one's)
  }
  head[i] = first ? 1u : 0u;
  agg[i] = { (uint32_t)f, rec, off, off, f == IVF_NO_FAMILY ? 0u : 1u };
}

int ivf_scan_heads(nts_ctx* ctx, uint32_t* d_head, uint32_t* d_id, uint64_t n)
{
  size_t tmp = 0;
  HIP_TRY(ctx, rocprim::inclusive_scan(nullptr, tmp, d_head, d_id, n, rocprim::plus<uint32_t>(), ctx->stream));
  NTS_WS(d_tmp, void*, "ivs_tmp", std::max<size_t>(tmp, 16));
  HIP_TRY(ctx, rocprim::inclusive_scan(d_tmp, tmp, d_head, d_id, n, rocprim::plus<uint32_t>(), ctx->stream));
  return NTS_OK;
}

int ivf_runs(nts_ctx* ctx, const uint64_t* d_in, uint64_t n, uint64_t* d_unique, uint32_t* d_cnt, uint64_t* d_num)
{
  size_t tmp = 0;
  HIP_TRY(ctx, rocprim::run_length_encode(nullptr, tmp, d_in, n, d_unique, d_cnt, d_num, ctx->stream));
  NTS_WS(d_tmp, void*, "ivs_tmp", std::max<size_t>(tmp, 16));
  HIP_TRY(ctx, rocprim::run_length_encode(d_tmp, tmp, d_in, n, d_unique, d_cnt, d_num, ctx->stream));
  return NTS_OK;
}

// the copy of `n` elements of a device array into a malloc'd host array (*host = NULL on any failure)
template <typename T>
int ivf_to_host(nts_ctx* ctx, const char* who, const T* d_src, uint64_t n, T** host)
{
  *host = (T*)malloc(n * sizeof(T));
  if (!*host) return fail(ctx, NTS_ENOMEM, std::string(who) + ": host memory for the result");
  hipError_t e = hipMemcpyAsync(*host, d_src, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t e_sync = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess || e_sync != hipSuccess) {
    free(*host);
    *host = nullptr;
  }
  HIP_TRY(ctx, e);
  HIP_TRY(ctx, e_sync);
  return NTS_OK;
}

int iv_period_hashes_run(nts_ctx* ctx, const nts_sample* recs, uint64_t n, uint64_t n_iv, const uint32_t* period, nts_sample** out, uint64_t* n_out)
{
  if (n > 0xFFFFFFFFull || n_iv > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_iv_period_hashes: 2^32 records or intervals or more (raise the rate)");
  if (int rc = ivp_check(ctx, "nts_iv_period_hashes", recs, n, n_iv)) return rc;
  if (n == 0 || n_iv == 0) return NTS_OK;
  NTS_WS(d_period, uint32_t*, "ivf_period", n_iv * 4);
  NTS_WS(d_head, uint32_t*, "ivf_head", n * 4);
  NTS_WS(d_rid, uint32_t*, "ivf_rid", n * 4);
  NTS_WS(d_urid, uint32_t*, "ivf_urid", n * 4);
  NTS_WS(d_val, nts_sample*, "ivf_val", n * sizeof(nts_sample));
  NTS_WS(d_uval, nts_sample*, "ivf_uval", n * sizeof(nts_sample));
  NTS_WS(d_num, uint64_t*, "ivf_num", 16);
  HIP_TRY(ctx, hipMemcpyAsync(d_period, period, n_iv * 4, hipMemcpyHostToDevice, ctx->stream));
  IvpLags B;
  if (int rc = ivp_lags(ctx, recs, n, "iv_phash", "iv_phash", &B)) return rc;
  uint64_t nu = 0;
  {
    ScopedTimer t(ctx, "iv_phash");
    NTS_LAUNCH(k_ivf_mark, IVL_GRID(n), (const uint64_t*)B.h, (const uint64_t*)B.v, (const uint32_t*)B.lag, n, (const uint32_t*)d_period, n_iv, d_head, d_val);
    if (int rc = ivf_scan_heads(ctx, d_head, d_rid, n)) return rc;
    size_t tmp = 0;
    HIP_TRY(ctx, rocprim::reduce_by_key(nullptr, tmp, d_rid, d_val, n, d_urid, d_uval, d_num, IvfCount(), rocprim::equal_to<uint32_t>(), ctx->stream));
    NTS_WS(d_tmp, void*, "ivs_tmp", std::max<size_t>(tmp, 16));
    HIP_TRY(ctx, rocprim::reduce_by_key(d_tmp, tmp, d_rid, d_val, n, d_urid, d_uval, d_num, IvfCount(), rocprim::equal_to<uint32_t>(), ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&nu, d_num, 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // (the caller's arrays are the caller's again from here)
  if (nu == 0 || nu > n) return fail(ctx, NTS_EHIP, "nts_iv_period_hashes: the per-run reduction returned an impossible count");
  uint64_t nk = 0;
  {
    ScopedTimer t(ctx, "iv_phash");
    size_t tmp = 0; // (d_val is free again: the kept runs)
    HIP_TRY(ctx, rocprim::select(nullptr, tmp, d_uval, d_val, d_num, nu, IvfHas(), ctx->stream));
    NTS_WS(d_tmp, void*, "ivs_tmp", std::max<size_t>(tmp, 16));
    HIP_TRY(ctx, rocprim::select(d_tmp, tmp, d_uval, d_val, d_num, nu, IvfHas(), ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&nk, d_num, 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (nk > nu) return fail(ctx, NTS_EHIP, "nts_iv_period_hashes: the selection returned an impossible count");
  if (nk == 0) return NTS_OK;
  if (int rc = ivf_to_host(ctx, "nts_iv_period_hashes", (const nts_sample*)d_val, nk, out)) return rc;
  *n_out = nk;
  return NTS_OK;
}

int iv_families_run(nts_ctx* ctx, const nts_sample* pairs, uint64_t n, uint64_t n_arrays, uint32_t* family, uint64_t** hashes, uint32_t** hash_family,
                    uint64_t* n_hashes)
{
  if (n > 0xFFFFFFFFull || n_arrays > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_iv_families: 2^32 pairs or arrays or more");
  for (uint64_t i = 0; i < n; ++i)
    if (pairs[i].iv >= n_arrays) return fail(ctx, NTS_EINVAL, "nts_iv_families: a pair names an array at or beyond n_arrays");
  for (uint64_t a = 0; a < n_arrays; ++a) family[a] = (uint32_t)a;
  if (n == 0) return NTS_OK;
  NTS_WS(d_pair, nts_sample*, "ivf_pair", n * sizeof(nts_sample));
  NTS_WS(d_h, uint64_t*, "ivf_h", n * 8);
  NTS_WS(d_a, uint64_t*, "ivf_a", n * 8);
  NTS_WS(d_h2, uint64_t*, "ivf_h2", n * 8);
  NTS_WS(d_a2, uint64_t*, "ivf_a2", n * 8);
  NTS_WS(d_edge, uint64_t*, "ivf_edge", n * 8);
  NTS_WS(d_ecnt, uint32_t*, "ivf_ecnt", n * 4);
  NTS_WS(d_hcnt, uint32_t*, "ivf_hcnt", n * 4);
  NTS_WS(d_at, uint64_t*, "ivf_at", n * 8);
  NTS_WS(d_first, uint32_t*, "ivf_first", n * 4);
  NTS_WS(d_num, uint64_t*, "ivf_num", 16);
  HIP_TRY(ctx, hipMemcpyAsync(d_pair, pairs, n * sizeof(nts_sample), hipMemcpyHostToDevice, ctx->stream));
  uint64_t num[2] = { 0, 0 };
  {
    ScopedTimer t(ctx, "iv_families_join");
    NTS_LAUNCH(k_ivf_split, IVL_GRID(n), (const nts_sample*)d_pair, n, d_h, d_a);
    if (int rc = ivs_sort(ctx, d_a, d_a2, d_h, d_h2, n, 32)) return rc;
    if (int rc = ivs_sort(ctx, d_h2, d_h, d_a2, d_a, n, 64)) return rc; // (stable: within a hash the iv order stays)
    NTS_LAUNCH(k_ivf_edges, IVL_GRID(n), (const uint64_t*)d_h, (const uint64_t*)d_a, n, d_edge);
    size_t tmp = 0; // (d_a2 is free again: the sorted edges; then d_edge: the distinct ones)
    HIP_TRY(ctx, rocprim::radix_sort_keys(nullptr, tmp, d_edge, d_a2, n, 0, 64, ctx->stream));
    {
      NTS_WS(d_tmp, void*, "ivs_tmp", std::max<size_t>(tmp, 16));
      HIP_TRY(ctx, rocprim::radix_sort_keys(d_tmp, tmp, d_edge, d_a2, n, 0, 64, ctx->stream));
    }
    if (int rc = ivf_runs(ctx, d_a2, n, d_edge, d_ecnt, d_num)) return rc;
    if (int rc = ivf_runs(ctx, d_h, n, d_h2, d_hcnt, d_num + 1)) return rc; // (d_h2 is free again: the distinct hashes)
    HIP_TRY(ctx, hipMemcpyAsync(num, d_num, 16, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // (the caller's array is the caller's again from here)
  const uint64_t ne = num[0] - 1, nh = num[1]; // (the run of IVF_NONE is the last one)
  if (num[0] == 0 || num[0] > n || nh == 0 || nh > n) return fail(ctx, NTS_EHIP, "nts_iv_families: the run-length encoding returned an impossible count");
  {
    ScopedTimer t(ctx, "iv_families_join");
    if (int rc = scan_counts(ctx, (const uint32_t*)d_hcnt, nh, d_at)) return rc;
    NTS_LAUNCH(k_ivf_first, IVL_GRID(nh), (const uint64_t*)d_a, n, (const uint64_t*)d_at, nh, d_first);
  }
  HIP_TRY(ctx, hipGetLastError());
  std::vector<uint64_t> edges(ne);
  if (ne) {
    const hipError_t e = hipMemcpyAsync(edges.data(), d_edge, ne * 8, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t e_sync = hipStreamSynchronize(ctx->stream); // (before anything below can return and take `edges` away)
    HIP_TRY(ctx, e);
    HIP_TRY(ctx, e_sync);
  }
  uint64_t* uh = nullptr;
  uint32_t* fam = nullptr;
  if (int rc = ivf_to_host(ctx, "nts_iv_families", (const uint64_t*)d_h2, nh, &uh)) return rc;
  if (int rc = ivf_to_host(ctx, "nts_iv_families", (const uint32_t*)d_first, nh, &fam)) {
    free(uh);
    return rc;
  }
  // ---- host: union-find, the smaller root wins, so a component's root is its smallest array
  auto root = [&](uint32_t a) {
    while (family[a] != a) {
      family[a] = family[family[a]];
      a = family[a];
    }
    return a;
  };
  bool bad = false;
  for (uint64_t e : edges) {
    const uint64_t x = e >> 32, y = e & 0xFFFFFFFFull;
    if (x >= n_arrays || y >= n_arrays) {
      bad = true;
      break;
    }
    const uint32_t rx = root((uint32_t)x), ry = root((uint32_t)y);
    if (rx < ry)
      family[ry] = rx;
    else if (ry < rx)
      family[rx] = ry;
  }
  for (uint64_t j = 0; j < nh && !bad; ++j) bad = fam[j] >= n_arrays;
  if (bad) {
    free(uh);
    free(fam);
    for (uint64_t a = 0; a < n_arrays; ++a) family[a] = (uint32_t)a;
    return fail(ctx, NTS_EHIP, "nts_iv_families: the device returned an array index beyond n_arrays");
  }
  for (uint64_t a = 0; a < n_arrays; ++a) family[a] = root((uint32_t)a);
  for (uint64_t j = 0; j < nh; ++j) fam[j] = family[fam[j]];
  *hashes = uh;
  *hash_family = fam;
  *n_hashes = nh;
  return NTS_OK;
}

int iv_family_sites_run(nts_ctx* ctx, const nts_sample* occ, uint64_t n, const uint64_t* hashes, const uint32_t* hash_family, uint64_t nh, uint32_t step,
                        uint32_t min_hits, nts_iv_fsite** out, uint64_t* n_out)
{
  if (n > 0xFFFFFFFFull || nh > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_iv_family_sites: 2^32 occurrences or hashes or more (raise the rate)");
  for (uint64_t i = 1; i < n; ++i)
    if (occ[i].iv < occ[i - 1].iv || (occ[i].iv == occ[i - 1].iv && occ[i].off <= occ[i - 1].off))
      return fail(ctx, NTS_EINVAL, "nts_iv_family_sites: the occurrences are not in (iv, off) order, off rising strictly within a record");
  for (uint64_t j = 1; j < nh; ++j)
    if (hashes[j] <= hashes[j - 1]) return fail(ctx, NTS_EINVAL, "nts_iv_family_sites: the hashes do not ascend strictly");
  if (n == 0 || nh == 0) return NTS_OK;
  NTS_WS(d_occ, nts_sample*, "ivf_pair", n * sizeof(nts_sample));
  NTS_WS(d_hashes, uint64_t*, "ivf_hashes", nh * 8);
  NTS_WS(d_hfam, uint32_t*, "ivf_hfam", nh * 4);
  NTS_WS(d_key, uint64_t*, "ivf_h", n * 8);
  NTS_WS(d_val, uint64_t*, "ivf_a", n * 8);
  NTS_WS(d_key2, uint64_t*, "ivf_h2", n * 8);
  NTS_WS(d_val2, uint64_t*, "ivf_a2", n * 8);
  NTS_WS(d_head, uint32_t*, "ivf_head", n * 4);
  NTS_WS(d_sid, uint32_t*, "ivf_rid", n * 4);
  NTS_WS(d_usid, uint32_t*, "ivf_urid", n * 4);
  NTS_WS(d_agg, nts_iv_fsite*, "ivf_agg", n * sizeof(nts_iv_fsite));
  NTS_WS(d_uagg, nts_iv_fsite*, "ivf_uagg", n * sizeof(nts_iv_fsite));
  NTS_WS(d_num, uint64_t*, "ivf_num", 16);
  HIP_TRY(ctx, hipMemcpyAsync(d_occ, occ, n * sizeof(nts_sample), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_hashes, hashes, nh * 8, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_hfam, hash_family, nh * 4, hipMemcpyHostToDevice, ctx->stream));
  uint64_t nu = 0;
  {
    ScopedTimer t(ctx, "iv_family_sites_label");
    NTS_LAUNCH(k_ivf_lookup, IVL_GRID(n), (const nts_sample*)d_occ, n, (const uint64_t*)d_hashes, (const uint32_t*)d_hfam, nh, d_key, d_val);
    if (int rc = ivs_sort(ctx, d_key, d_key2, d_val, d_val2, n, 33)) return rc; // (stable: within a family the (rec, off) order stays)
    NTS_LAUNCH(k_ivf_breaks, IVL_GRID(n), (const uint64_t*)d_key2, (const uint64_t*)d_val2, n, step, d_head, d_agg);
    if (int rc = ivf_scan_heads(ctx, d_head, d_sid, n)) return rc;
    size_t tmp = 0;
    HIP_TRY(ctx, rocprim::reduce_by_key(nullptr, tmp, d_sid, d_agg, n, d_usid, d_uagg, d_num, IvfAdd(), rocprim::equal_to<uint32_t>(), ctx->stream));
    NTS_WS(d_tmp, void*, "ivs_tmp", std::max<size_t>(tmp, 16));
    HIP_TRY(ctx, rocprim::reduce_by_key(d_tmp, tmp, d_sid, d_agg, n, d_usid, d_uagg, d_num, IvfAdd(), rocprim::equal_to<uint32_t>(), ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&nu, d_num, 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // (the caller's arrays are the caller's again from here)
  if (nu == 0 || nu > n) return fail(ctx, NTS_EHIP, "nts_iv_family_sites: the per-site reduction returned an impossible count");
  uint64_t nk = 0;
  {
    ScopedTimer t(ctx, "iv_family_sites_select");
    size_t tmp = 0; // (d_agg is free again: the kept sites)
    HIP_TRY(ctx, rocprim::select(nullptr, tmp, d_uagg, d_agg, d_num, nu, IvfKeep{ min_hits }, ctx->stream));
    NTS_WS(d_tmp, void*, "ivs_tmp", std::max<size_t>(tmp, 16));
    HIP_TRY(ctx, rocprim::select(d_tmp, tmp, d_uagg, d_agg, d_num, nu, IvfKeep{ min_hits }, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&nk, d_num, 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (nk > nu) return fail(ctx, NTS_EHIP, "nts_iv_family_sites: the selection returned an impossible count");
  if (nk == 0) return NTS_OK;
  if (int rc = ivf_to_host(ctx, "nts_iv_family_sites", (const nts_iv_fsite*)d_agg, nk, out)) return rc;
  *n_out = nk;
  return NTS_OK;
}

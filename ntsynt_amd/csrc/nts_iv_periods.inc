// ---- the dominant lag between the recurrences of a hash inside each interval of ONE list of sampled records (nts_iv_periods; ----
// ntsynt_amd/gaps.py periods).  docs/design/04_14_gap_periods.md.  Sampling is by hash value, so a k-mer that recurs is sampled at every
// recurrence or at none: the records of one interval with equal h0, in order of off, carry the exact distances between consecutive
// copies of that k-mer.  In a tandem array most of them are one unit apart: the lag held by the most records is the period.
// All on the context's stream and in its workspace, no atomic, no launch per interval, no floating point:
//   1  k_ivp_split: h0 and off << 32 | iv of every record (the records arrive in (iv, off) order)
//   2  stable radix sort by h0 carrying off | iv, then stable sort by the LOWER 32 bits of off | iv (the interval: bits 0..32, as
//      nts_iv_sites step 5 sorts its gap ids and for its reason) carrying h0: (iv, h0, off) order, no permutation array
//   3  k_ivp_lags: one lane per record; it has a lag when its predecessor has the same iv and h0: lag = off - the predecessor's off
//      (>= 1: off rises strictly within an interval).  It stores the key iv << 32 | lag, or IVP_NONE (iv < 2^32 - 1: no key equals it),
//      and the lag itself (0 = none) for step 6
//   4  radix sort of the keys; rocprim::run_length_encode turns them into (iv, lag, count), lags ascending within an interval, the run
//      of IVP_NONE last
//   5  one rocprim::reduce_by_key over iv: the counts add up to `recurring`; of two runs the one with the larger count stays, the
//      earlier (smaller lag) on a tie.  k_ivp_modes stores {recurring, period, period_hits} at out[iv] (out was cleared: an interval
//      without a record, or without a recurrence, keeps its zeros)
//   6  k_ivp_extent: one lane per record of step 2's order; a record whose lag is its interval's period gives (off - lag, off), any
//      other the identity of (min, max); one rocprim::reduce_by_key over iv; k_ivp_extents stores first_off / last_off at out[iv]
// Steps 1 - 3 are the helper ivp_lags and the order check is ivp_check: nts_iv_period_hashes (nts_iv_families.inc) starts from the same
// (iv, h0, off) order and the same lags.
// The two scatter kernels read how many keys the reductions produced from device memory; the host needs only the number of runs of
// step 4 (one synchronise), which is also where the caller's array is the caller's again.

constexpr uint64_t IVP_NONE = ~0ULL;

struct IvpMode
{
  uint32_t recurring, hits, lag;
};

struct IvpBest // (runs arrive by ascending lag within an interval: on a tie the left one has the smaller lag, compared all the same)
{
  __host__ __device__ IvpMode operator()(const IvpMode& x, const IvpMode& y) const
  {
    const bool left = x.hits > y.hits || (x.hits == y.hits && x.lag <= y.lag);
    return { x.recurring + y.recurring, left ? x.hits : y.hits, left ? x.lag : y.lag };
  }
};

struct IvpExt // lo > hi: no record yet
{
  uint32_t lo, hi;
};

struct IvpSpan
{
  __host__ __device__ IvpExt operator()(const IvpExt& x, const IvpExt& y) const { return { x.lo < y.lo ? x.lo : y.lo, x.hi > y.hi ? x.hi : y.hi }; }
};

struct IvpLow32 // the interval of an off | iv word
{
  __host__ __device__ uint32_t operator()(uint64_t v) const { return (uint32_t)v; }
};
static_assert(sizeof(nts_iv_period) == 20, "the C ABI's layout");

__global__ __launch_bounds__(256) void k_ivp_split(const nts_sample* __restrict__ rec, uint64_t n, uint64_t* __restrict__ h, uint64_t* __restrict__ v)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const nts_sample r = rec[i];
  h[i] = r.h0;
  v[i] = ((uint64_t)r.off << 32) | r.iv;
}

// records in (iv, h0, off) order
__global__ __launch_bounds__(256) void k_ivp_lags(const uint64_t* __restrict__ h, const uint64_t* __restrict__ v, uint64_t n, uint64_t* __restrict__ key,
                                                  uint32_t* __restrict__ lag)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t w = v[i];
  uint32_t d = 0;
  if (i > 0) {
    const uint64_t pw = v[i - 1];
    if ((uint32_t)pw == (uint32_t)w && h[i - 1] == h[i]) d = (uint32_t)(w >> 32) - (uint32_t)(pw >> 32);
  }
  key[i] = d ? ((w << 32) | d) : IVP_NONE;
  lag[i] = d;
}

// run j of the sorted keys: its interval and what it brings to the interval's mode
__global__ __launch_bounds__(256) void k_ivp_runs(const uint64_t* __restrict__ ukey, const uint32_t* __restrict__ cnt, uint64_t nr, uint32_t* __restrict__ iv,
                                                  IvpMode* __restrict__ mode)
{
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nr) return;
  const uint64_t key = ukey[j];
  iv[j] = (uint32_t)(key >> 32);
  mode[j] = key == IVP_NONE ? IvpMode{ 0u, 0u, 0u } : IvpMode{ cnt[j], cnt[j], (uint32_t)key };
}

__global__ __launch_bounds__(256) void k_ivp_modes(const uint32_t* __restrict__ iv, const IvpMode* __restrict__ mode, const uint64_t* __restrict__ n_keys,
                                                   uint64_t cap, uint64_t n_iv, nts_iv_period* __restrict__ out)
{
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cap || j >= *n_keys) return;
  const uint32_t i = iv[j];
  const IvpMode m = mode[j];
  if (i >= n_iv || m.hits == 0) return; // (the run of IVP_NONE: interval 2^32 - 1)
  out[i].recurring = m.recurring;
  out[i].period = m.lag;
  out[i].period_hits = m.hits;
}

__global__ __launch_bounds__(256) void k_ivp_extent(const uint64_t* __restrict__ v, const uint32_t* __restrict__ lag, uint64_t n, uint64_t n_iv,
                                                    const nts_iv_period* __restrict__ out, IvpExt* __restrict__ ext)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t w = v[i];
  const uint32_t iv = (uint32_t)w, off = (uint32_t)(w >> 32), d = lag[i];
  IvpExt e{ 0xFFFFFFFFu, 0u };
  if (d && iv < n_iv && out[iv].period == d) e = { off - d, off };
  ext[i] = e;
}

__global__ __launch_bounds__(256) void k_ivp_extents(const uint32_t* __restrict__ iv, const IvpExt* __restrict__ ext, const uint64_t* __restrict__ n_keys,
                                                     uint64_t cap, uint64_t n_iv, nts_iv_period* __restrict__ out)
{
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cap || j >= *n_keys) return;
  const uint32_t i = iv[j];
  const IvpExt e = ext[j];
  if (i >= n_iv || e.lo > e.hi) return;
  out[i].first_off = e.lo;
  out[i].last_off = e.hi;
}

// the order a sampler's records have, checked in one pass (`who`: the call the message names)
int ivp_check(nts_ctx* ctx, const char* who, const nts_sample* recs, uint64_t n, uint64_t n_iv)
{
  for (uint64_t i = 0; i < n; ++i) {
    if (recs[i].iv >= n_iv) return fail(ctx, NTS_EINVAL, std::string(who) + ": a record names an interval at or beyond n_iv");
    if (i && (recs[i].iv < recs[i - 1].iv || (recs[i].iv == recs[i - 1].iv && recs[i].off <= recs[i - 1].off)))
      return fail(ctx, NTS_EINVAL, std::string(who) + ": the records are not in (iv, off) order, off rising strictly within an interval");
  }
  return NTS_OK;
}

// steps 1 - 3 for nts_iv_periods and nts_iv_period_hashes (nts_iv_families.inc): h, v = the records' h0 and off << 32 | iv in
// (iv, h0, off) order, lag = each record's lag (0 = none), h2 = the keys of step 3, v2 = free; all n long, in the workspace
struct IvpLags
{
  uint64_t *h, *v, *h2, *v2;
  uint32_t* lag;
};

int ivp_lags(nts_ctx* ctx, const nts_sample* recs, uint64_t n, const char* t_sort, const char* t_lags, IvpLags* B)
{
  NTS_WS(d_rec, nts_sample*, "ivp_rec", n * sizeof(nts_sample));
  NTS_WS(d_h, uint64_t*, "ivp_h", n * 8);
  NTS_WS(d_v, uint64_t*, "ivp_v", n * 8);
  NTS_WS(d_h2, uint64_t*, "ivp_h2", n * 8);
  NTS_WS(d_v2, uint64_t*, "ivp_v2", n * 8);
  NTS_WS(d_lag, uint32_t*, "ivp_lag", n * 4);
  HIP_TRY(ctx, hipMemcpyAsync(d_rec, recs, n * sizeof(nts_sample), hipMemcpyHostToDevice, ctx->stream));
  {
    ScopedTimer t(ctx, t_sort);
    NTS_LAUNCH(k_ivp_split, IVL_GRID(n), (const nts_sample*)d_rec, n, d_h, d_v);
    if (int rc = ivs_sort(ctx, d_h, d_h2, d_v, d_v2, n, 64)) return rc;
    if (int rc = ivs_sort(ctx, d_v2, d_v, d_h2, d_h, n, 32)) return rc; // (by the interval only: within one the (h0, off) order stays)
  }
  {
    ScopedTimer t(ctx, t_lags);
    // (d_h2 and d_v2 are free again: the lag keys and, for the caller, their sorted copy)
    NTS_LAUNCH(k_ivp_lags, IVL_GRID(n), (const uint64_t*)d_h, (const uint64_t*)d_v, n, d_h2, d_lag);
  }
  *B = { d_h, d_v, d_h2, d_v2, d_lag };
  return NTS_OK;
}

int iv_periods_run(nts_ctx* ctx, const nts_sample* recs, uint64_t n, uint64_t n_iv, nts_iv_period* out)
{
  if (n > 0xFFFFFFFFull || n_iv > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_iv_periods: 2^32 records or intervals or more (raise the rate)");
  if (int rc = ivp_check(ctx, "nts_iv_periods", recs, n, n_iv)) return rc;
  if (n_iv) memset(out, 0, n_iv * sizeof(nts_iv_period));
  if (n == 0 || n_iv == 0) return NTS_OK;
  NTS_WS(d_cnt, uint32_t*, "ivp_cnt", n * 4);
  NTS_WS(d_riv, uint32_t*, "ivp_riv", n * 4);
  NTS_WS(d_uiv, uint32_t*, "ivp_uiv", n * 4);
  NTS_WS(d_mode, IvpMode*, "ivp_mode", n * sizeof(IvpMode));
  NTS_WS(d_umode, IvpMode*, "ivp_umode", n * sizeof(IvpMode));
  NTS_WS(d_ext, IvpExt*, "ivp_ext", n * sizeof(IvpExt));
  NTS_WS(d_uext, IvpExt*, "ivp_uext", n * sizeof(IvpExt));
  NTS_WS(d_num, uint64_t*, "ivp_num", 8);
  NTS_WS(d_out, nts_iv_period*, "ivp_out", n_iv * sizeof(nts_iv_period));
  HIP_TRY(ctx, hipMemsetAsync(d_out, 0, n_iv * sizeof(nts_iv_period), ctx->stream));
  IvpLags B;
  if (int rc = ivp_lags(ctx, recs, n, "iv_periods_sort", "iv_periods_mode", &B)) return rc;
  uint64_t* const d_h2 = B.h2;
  uint64_t* const d_v2 = B.v2;
  const uint64_t* const d_v = B.v;
  const uint32_t* const d_lag = B.lag;
  uint64_t nr = 0;
  {
    ScopedTimer t(ctx, "iv_periods_mode");
    size_t tmp = 0;
    HIP_TRY(ctx, rocprim::radix_sort_keys(nullptr, tmp, d_h2, d_v2, n, 0, 64, ctx->stream));
    {
      NTS_WS(d_tmp, void*, "ivs_tmp", std::max<size_t>(tmp, 16));
      HIP_TRY(ctx, rocprim::radix_sort_keys(d_tmp, tmp, d_h2, d_v2, n, 0, 64, ctx->stream));
    }
    tmp = 0; // (d_h2 is free once more: the runs' keys)
    HIP_TRY(ctx, rocprim::run_length_encode(nullptr, tmp, d_v2, n, d_h2, d_cnt, d_num, ctx->stream));
    NTS_WS(d_tmp, void*, "ivs_tmp", std::max<size_t>(tmp, 16));
    HIP_TRY(ctx, rocprim::run_length_encode(d_tmp, tmp, d_v2, n, d_h2, d_cnt, d_num, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&nr, d_num, 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // (the caller's array is the caller's again from here)
  if (nr == 0 || nr > n) return fail(ctx, NTS_EHIP, "nts_iv_periods: the run-length encoding returned an impossible count");
  {
    ScopedTimer t(ctx, "iv_periods_mode");
    NTS_LAUNCH(k_ivp_runs, IVL_GRID(nr), (const uint64_t*)d_h2, (const uint32_t*)d_cnt, nr, d_riv, d_mode);
    size_t tmp = 0;
    HIP_TRY(ctx, rocprim::reduce_by_key(nullptr, tmp, d_riv, d_mode, nr, d_uiv, d_umode, d_num, IvpBest(), rocprim::equal_to<uint32_t>(), ctx->stream));
    NTS_WS(d_tmp, void*, "ivs_tmp", std::max<size_t>(tmp, 16));
    HIP_TRY(ctx, rocprim::reduce_by_key(d_tmp, tmp, d_riv, d_mode, nr, d_uiv, d_umode, d_num, IvpBest(), rocprim::equal_to<uint32_t>(), ctx->stream));
    NTS_LAUNCH(k_ivp_modes, IVL_GRID(nr), (const uint32_t*)d_uiv, (const IvpMode*)d_umode, (const uint64_t*)d_num, nr, n_iv, d_out);
  }
  {
    ScopedTimer t(ctx, "iv_periods_extent");
    NTS_LAUNCH(k_ivp_extent, IVL_GRID(n), d_v, d_lag, n, n_iv, (const nts_iv_period*)d_out, d_ext);
    auto keys = rocprim::make_transform_iterator(d_v, IvpLow32());
    size_t tmp = 0;
    HIP_TRY(ctx, rocprim::reduce_by_key(nullptr, tmp, keys, d_ext, n, d_uiv, d_uext, d_num, IvpSpan(), rocprim::equal_to<uint32_t>(), ctx->stream));
    NTS_WS(d_tmp, void*, "ivs_tmp", std::max<size_t>(tmp, 16));
    HIP_TRY(ctx, rocprim::reduce_by_key(d_tmp, tmp, keys, d_ext, n, d_uiv, d_uext, d_num, IvpSpan(), rocprim::equal_to<uint32_t>(), ctx->stream));
    NTS_LAUNCH(k_ivp_extents, IVL_GRID(n), (const uint32_t*)d_uiv, (const IvpExt*)d_uext, (const uint64_t*)d_num, n, n_iv, d_out);
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(out, d_out, n_iv * sizeof(nts_iv_period), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return NTS_OK;
}

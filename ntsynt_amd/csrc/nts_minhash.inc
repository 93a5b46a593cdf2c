// ---- bottom-s MinHash sketch of a genome's distinct canonical k-mer hashes (nts_minhash; ntsynt_amd/divergence.py) ----------
// One sweep of k_hash<MODE_MINHASH> over the run table: every valid k-mer with h0 < tau joins a device open-addressing set
// (MhSet, next to k_hash), which removes copies across the whole genome -- a satellite in 10^6 copies is one entry.  The sketch is
// exact: once a sweep leaves between s and cap / 2 distinct hashes in the set, the set holds every distinct hash below tau, so its
// s smallest are the genome's s smallest.
//   tau: starts at 4 s 2^64 / n_valid (about 4 s survivors when the k-mers are distinct).  Too few distinct survivors (< s) and
//        tau < 2^64 - 1: raise it; more than cap / 2: lower it.  The distinct count is monotone in tau and steps by one, so the
//        window [s, cap / 2] (cap >= 4 s) is never empty, and every retry narrows a bracket (lo, hi) -- the loop ends.
//   cap: max(2^22, 64 s) slots, at least 4 s, a power of two.  Survivors are compacted on the device; the host sorts them (at
//        most cap / 2) and keeps the first s.
// Experiments build only: NTS_MINHASH_TAU0 = the first tau, NTS_MINHASH_CAP = the capacity (clamped as above) -- the tests force
// both retry directions with them on small genomes.

__global__ __launch_bounds__(256) void k_mh_compact(const uint64_t* __restrict__ slots, uint64_t cap, uint64_t* __restrict__ out,
                                                    uint64_t n_max, unsigned long long* __restrict__ cursor)
{
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= cap) return;
  const uint64_t v = slots[i];
  if (v == KEY_MAX) return;
  const unsigned long long at = atomicAdd(cursor, 1ULL);
  if (at < n_max) out[at] = v;
}

uint64_t mh_pow2_at_least(uint64_t x)
{
  uint64_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

// the s smallest distinct h0 of g (ascending) into `out`; *n_out = how many (fewer than s if g has fewer distinct valid k-mers)
// (each sweep is one launch of the timer "minhash": nts_timing counts the sweeps when profiling is on)
int minhash_run(nts_ctx* ctx, const nts_genome* g, uint32_t k, uint32_t s, uint64_t* out, uint32_t* n_out)
{
  GenomeTables scratch;
  const GenomeTables* T = nullptr;
  int rc = get_tables(ctx, g, k, nullptr, 0, scratch, &T);
  if (rc) return rc;
  const uint64_t n_valid = T->rt.n_valid;
  *n_out = 0;
  if (n_valid == 0) return NTS_OK;
  using u128 = unsigned __int128;
  const u128 TOP = (u128)KEY_MAX; // tau never exceeds it: h0 == KEY_MAX is the empty slot and never survives
  uint64_t cap = std::max<uint64_t>((uint64_t)1 << 22, (uint64_t)64 * s);
  if (const char* v = NTS_KNOB("NTS_MINHASH_CAP")) cap = strtoull(v, nullptr, 0);
  cap = mh_pow2_at_least(std::max<uint64_t>(cap, (uint64_t)4 * s));
  const uint64_t limit = cap / 2;
  u128 tau = ((u128)4 * s << 64) / n_valid;
  if (const char* v = NTS_KNOB("NTS_MINHASH_TAU0")) tau = (u128)strtoull(v, nullptr, 0);
  tau = std::min(std::max(tau, (u128)1), TOP);
  uint64_t* d_slots = nullptr;
  unsigned long long* d_count = nullptr; // [0] distinct survivors, [1] compaction cursor
  HIP_TRY(ctx, dev_malloc((void**)&d_slots, cap * 8));
  if (hipError_t e = dev_malloc((void**)&d_count, 16); e != hipSuccess) {
    dev_free(d_slots);
    HIP_TRY(ctx, e);
  }
  auto release = [&]() {
    hipStreamSynchronize(ctx->stream);
    dev_free(d_slots);
    dev_free(d_count);
  };
  u128 lo = 0, hi = TOP + 1; // count(lo) < s, count(hi) > limit (hi = 2^64: not known yet)
  unsigned long long count = 0;
  for (;;) {
    hipError_t e = hipMemsetAsync(d_slots, 0xFF, cap * 8, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_count, 0, 16, ctx->stream);
    if (e != hipSuccess) {
      release();
      HIP_TRY(ctx, e);
    }
    MhSet mh;
    mh.slots = d_slots;
    mh.count = d_count;
    mh.mask = cap - 1;
    mh.limit = limit;
    mh.tau = (uint64_t)tau;
    rc = launch_hash<MODE_MINHASH>(ctx, "minhash", g, *T, k, nullptr, nullptr, nullptr, nullptr, 0, nullptr, mh);
    if (rc == NTS_OK) {
      e = hipMemcpyAsync(&count, d_count, 8, hipMemcpyDeviceToHost, ctx->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    if (rc != NTS_OK || e != hipSuccess) {
      release();
      if (rc != NTS_OK) return rc;
      HIP_TRY(ctx, e);
    }
    if (count > limit) { // too many: lower tau, aiming at a quarter of the capacity
      hi = tau;
      u128 nt = tau * (u128)(limit / 2) / (u128)count;
      if (nt <= lo || nt >= hi) nt = lo + (hi - lo) / 2;
      tau = nt;
    } else if (count < s && tau < TOP) { // too few: raise tau, aiming at 4 s
      lo = tau;
      u128 nt = count ? tau * (u128)(4 * (uint64_t)s) / (u128)count : tau * 16;
      if (nt > TOP) nt = TOP;
      if (nt <= lo || nt >= hi) nt = lo + (hi - lo) / 2;
      tau = nt;
    } else {
      break;
    }
    if (tau <= lo || tau >= hi) { // cannot happen while count steps by one (see above); never loop on it
      release();
      return fail(ctx, NTS_ERANGE, "nts_minhash: the threshold bracket closed without a sketch");
    }
  }
  std::vector<uint64_t> host(count);
  if (count) {
    uint64_t* d_out = nullptr;
    hipError_t e = dev_malloc((void**)&d_out, count * 8);
    if (e == hipSuccess) {
      NTS_LAUNCH(k_mh_compact, dim3((uint32_t)((cap + 255) / 256)), dim3(256), 0, ctx->stream, d_slots, cap, d_out, (uint64_t)count,
                 d_count + 1);
      e = hipGetLastError();
      if (e == hipSuccess) e = hipMemcpyAsync(host.data(), d_out, count * 8, hipMemcpyDeviceToHost, ctx->stream);
      hipStreamSynchronize(ctx->stream);
      dev_free(d_out);
    }
    if (e != hipSuccess) {
      release();
      HIP_TRY(ctx, e);
    }
  }
  release();
  std::sort(host.begin(), host.end());
  const uint32_t n = (uint32_t)std::min<uint64_t>(s, host.size());
  std::copy(host.begin(), host.begin() + n, out);
  *n_out = n;
  return NTS_OK;
}

// ---- bottom-s MinHash sketches of many intervals of a resident genome (nts_minhash_intervals; ntsynt_amd/assess.py) -------------
// One sweep serves every interval of a call (docs/design/04_8_block_assessment.md).  The host cuts the intervals into tiles of valid
// k-mers (nts_iv_cut.inc); a workgroup sweeps one tile (nts_tile_sweep.inc) and inserts what the tile's interval keeps.
//   survivors: per-interval open-addressing sets (MhSet, next to k_hash; mhi_insert below), NOT an (interval, h0) list sorted and made
//        unique afterwards: a set removes copies where they arise, so that a satellite array -- 10^5 k-mers, a few hundred distinct
//        hashes, all of them below any threshold that keeps s of them -- fills a few hundred slots; in a list its copies overflow
//        whatever capacity the distinct count would justify, and no threshold has both "the list fits" and "s distinct survive".
//   tau_i: 4 s 2^64 / n_i (n_i = the interval's k-mers), KEY_MAX when n_i <= 4 s: short blocks keep everything.
//   cap_i: the smallest power of two >= max(64, min(4 n_i, 16 s)) slots; the interval is settled when its distinct count is within
//        [s, cap_i / 2], or below s with tau_i = KEY_MAX (it has fewer than s distinct hashes).  With tau_i = KEY_MAX and n_i <= 4 s
//        the count cannot pass cap_i / 4.  Otherwise cap_i / 2 >= 8 s: the window [s, cap_i / 2] is never empty, the count is monotone
//        in tau and steps by one, and every retry narrows the interval's own bracket (lo_i, hi_i) -- nts_minhash's rule, per interval.
//        A pass sweeps the tiles of the unsettled intervals only.  A closed bracket ends the call with NTS_ERANGE.
//   memory per interval: 8 cap_i bytes of slots (at most 256 s, 128 KB at s = 1000), 40 bytes of state, 16 bytes per distinct survivor
//        for the compacted and the sorted list (about 64 s), 8 s for the result.  The intervals of a call are served in chunks whose
//        slots stay within a budget (2 GiB; experiments build: NTS_MINHASH_IV_BUDGET).
//   the end of a chunk: the sets are compacted into one list, interval after interval, sorted by rocprim's segmented radix sort, and
//        the first min(s, count_i) of each segment are gathered and copied to the host in one piece.
// Experiments build only: NTS_MINHASH_TAU0 = the first tau of every interval, NTS_MINHASH_CAP = the slots of every interval (raised to
// 4 s and to a power of two): the tests force both retry directions with them.

struct MhiState
{
  uint64_t tau, slot_off, mask, limit;
};

// mh_insert for the sweep below: the same set, but what it would add to the interval's counter is returned (1: a new hash, cap: the
// probe walked the whole table, 0: present already) -- the tile adds its sum with ONE atomic.  A counter bumped per survivor is 4 s
// atomics on one address per interval, 4 10^7 per 10^4 blocks, and they ran one after the other: 131 ms per 3 Gbp (measured) for a
// sweep whose hashing takes 3.
__device__ __forceinline__ unsigned long long mhi_insert(const MhSet& mh, uint64_t h)
{
  uint64_t i = h & mh.mask;
  for (uint64_t probe = 0; probe <= mh.mask; ++probe) {
    const uint64_t cur = mh.slots[i];
    if (cur == h) return 0;
    if (cur == KEY_MAX) {
      const unsigned long long prev = atomicCAS(reinterpret_cast<unsigned long long*>(mh.slots + i), (unsigned long long)KEY_MAX,
                                                (unsigned long long)h);
      if (prev == KEY_MAX) return 1;
      if (prev == h) return 0;
    }
    i = (i + 1) & mh.mask;
  }
  return (unsigned long long)mh.mask + 1ULL;
}

constexpr uint32_t MHI_SUB = 8; // workgroups per interval of the small kernels (reset, compact, take)

__global__ __launch_bounds__(HASH_THREADS) void k_minhash_intervals(const uint8_t* __restrict__ code, const IvTile* __restrict__ tiles,
                                                                    const MhiState* __restrict__ state, uint64_t* __restrict__ slots,
                                                                    unsigned long long* __restrict__ counts, HashParams hp)
{
  __shared__ uint64_t s_tab[36];
  __shared__ uint32_t s_seq[SEQ_LDS_DWORDS];
  __shared__ unsigned long long s_added;
  if (threadIdx.x == 0) s_added = 0;
  const IvTile tile = tiles[blockIdx.x];
  const MhiState st = state[tile.iv];
  MhSet mh;
  mh.slots = slots + st.slot_off;
  mh.count = counts + tile.iv;
  mh.mask = st.mask;
  mh.limit = st.limit;
  mh.tau = st.tau;
  // an interval whose count is past its limit already is swept again with a lower tau: its remaining tiles of this pass do nothing
  // (the whole workgroup leaves: the value is read once, by a load every lane shares)
  if (__hip_atomic_load(mh.count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > mh.limit) return;
  const TileLane lane = tile_enter(s_tab, s_seq, code, tile.pos, tile.len, hp);
  unsigned long long added = 0;
  uint64_t h[8];
  lane.sweep(
    hp, s_tab, [&](uint32_t, int u, uint64_t h0) { h[u] = h0; },
    [&](uint32_t b0) { // (the inserts behind the batch's hashing: their probe loops diverge)
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (b0 + u < lane.n_mine && h[u] < mh.tau) added += mhi_insert(mh, h[u]);
    });
  // ---- the tile's new hashes onto the interval's counter: one atomic per workgroup
  if (added) atomicAdd(&s_added, added);
  __syncthreads();
  if (threadIdx.x == 0 && s_added) atomicAdd(mh.count, s_added);
}

// the sets and counts of the listed intervals back to empty (a retry pass)
__global__ __launch_bounds__(256) void k_mhi_reset(const uint32_t* __restrict__ list, const MhiState* __restrict__ state, uint64_t* __restrict__ slots,
                                                   unsigned long long* __restrict__ counts)
{
  const uint32_t iv = list[blockIdx.x / MHI_SUB], sub = blockIdx.x % MHI_SUB;
  const MhiState st = state[iv];
  for (uint64_t i = (uint64_t)sub * 256 + threadIdx.x; i <= st.mask; i += (uint64_t)MHI_SUB * 256) slots[st.slot_off + i] = KEY_MAX;
  if (sub == 0 && threadIdx.x == 0) counts[iv] = 0;
}

// the hashes of every interval's set into list[off[iv] ..), in any order (counts[iv] of them: the sets are settled)
__global__ __launch_bounds__(256) void k_mhi_compact(const MhiState* __restrict__ state, const uint64_t* __restrict__ slots, const uint64_t* __restrict__ off,
                                                     unsigned long long* __restrict__ cursor, uint64_t* __restrict__ list)
{
  const uint32_t iv = blockIdx.x / MHI_SUB, sub = blockIdx.x % MHI_SUB;
  const MhiState st = state[iv];
  const uint64_t o = off[iv], room = off[iv + 1] - o;
  for (uint64_t i = (uint64_t)sub * 256 + threadIdx.x; i <= st.mask; i += (uint64_t)MHI_SUB * 256) {
    const uint64_t v = slots[st.slot_off + i];
    if (v == KEY_MAX) continue;
    const unsigned long long at = atomicAdd(cursor + iv, 1ULL);
    if (at < room) list[o + at] = v;
  }
}

// the first take_off[iv + 1] - take_off[iv] hashes of every sorted segment, packed
__global__ __launch_bounds__(256) void k_mhi_take(const uint64_t* __restrict__ sorted, const uint64_t* __restrict__ off, const uint64_t* __restrict__ take_off,
                                                  uint64_t* __restrict__ out)
{
  const uint32_t iv = blockIdx.x / MHI_SUB, sub = blockIdx.x % MHI_SUB;
  const uint64_t o = off[iv], t = take_off[iv], n = take_off[iv + 1] - t;
  for (uint64_t i = (uint64_t)sub * 256 + threadIdx.x; i < n; i += (uint64_t)MHI_SUB * 256) out[t + i] = sorted[o + i];
}

// one chunk of intervals [i0, i1): pieces[piece_at[i] .. piece_at[i + 1]) are interval i's runs of k-mers, nk[i] their sum
int minhash_intervals_chunk(nts_ctx* ctx, const nts_genome* g, const HashParams& hp, uint32_t s, uint64_t i0, uint64_t i1,
                            const std::vector<IvPiece>& pieces, const std::vector<uint64_t>& piece_at, const std::vector<uint64_t>& nk,
                            const std::vector<uint64_t>& caps, uint64_t* out, uint32_t* n_out, uint32_t* passes_out)
{
  using u128 = unsigned __int128;
  const u128 TOP = (u128)KEY_MAX;
  const uint32_t n = (uint32_t)(i1 - i0);
  std::vector<MhiState> st(n);
  std::vector<u128> lo(n, 0), hi(n, TOP + 1);
  uint64_t n_slots = 0;
  for (uint32_t j = 0; j < n; ++j) {
    const uint64_t nv = nk[i0 + j];
    u128 tau = nv > (uint64_t)4 * s ? ((u128)4 * s << 64) / nv : TOP;
    if (const char* v = NTS_KNOB("NTS_MINHASH_TAU0")) tau = (u128)strtoull(v, nullptr, 0);
    tau = std::min(std::max(tau, (u128)1), TOP);
    st[j].tau = (uint64_t)tau;
    st[j].slot_off = n_slots;
    st[j].mask = caps[i0 + j] - 1;
    st[j].limit = caps[i0 + j] / 2;
    n_slots += caps[i0 + j];
  }
  NTS_WS(d_state, MhiState*, "mhi_state", (size_t)n * sizeof(MhiState));
  NTS_WS(d_counts, unsigned long long*, "mhi_counts", (size_t)n * 8);
  NTS_WS(d_retry, uint32_t*, "mhi_retry", (size_t)n * 4);
  uint64_t* d_slots = nullptr;
  uint64_t *d_list = nullptr, *d_sorted = nullptr, *d_take = nullptr;
  void* d_tmp = nullptr;
  auto release = [&]() {
    hipStreamSynchronize(ctx->stream);
    dev_free(d_slots);
    dev_free(d_list);
    dev_free(d_sorted);
    dev_free(d_take);
    dev_free(d_tmp);
  };
#define MHI_HIP(expr)                  \
  do {                                 \
    const hipError_t e__ = (expr);     \
    if (e__ != hipSuccess) {           \
      release();                       \
      HIP_TRY(ctx, e__);               \
    }                                  \
  } while (0)
#define MHI_RC(expr)                   \
  do {                                 \
    const int rc__ = (expr);           \
    if (rc__ != NTS_OK) {              \
      release();                       \
      return rc__;                     \
    }                                  \
  } while (0)
  MHI_HIP(dev_malloc((void**)&d_slots, std::max<uint64_t>(n_slots, 1) * 8));
  MHI_HIP(hipMemsetAsync(d_slots, 0xFF, std::max<uint64_t>(n_slots, 1) * 8, ctx->stream));
  MHI_HIP(hipMemsetAsync(d_counts, 0, (size_t)n * 8, ctx->stream));
  std::vector<uint32_t> active(n), retry;
  for (uint32_t j = 0; j < n; ++j) active[j] = j;
  std::vector<unsigned long long> counts(n, 0);
  std::vector<IvTile> tiles;
  uint32_t passes = 0;
  while (!active.empty()) {
    tiles.clear();
    for (uint32_t j : active) iv_append_tiles(pieces, piece_at, i0 + j, j, tiles);
    MHI_HIP(hipMemcpyAsync(d_state, st.data(), (size_t)n * sizeof(MhiState), hipMemcpyHostToDevice, ctx->stream));
    if (!tiles.empty()) {
      IvTile* d_tiles = nullptr;
      MHI_RC(ws_upload(ctx, "mhi_tiles", tiles, &d_tiles));
      iv_for_slices(ctx, "minhash_iv", tiles.size(), iv_slice(nullptr), [&](uint64_t t0, uint32_t nt) {
        NTS_LAUNCH(k_minhash_intervals, dim3(nt), dim3(HASH_THREADS), 0, ctx->stream, g->d_code + PAD, d_tiles + t0, d_state, d_slots, d_counts, hp);
      });
      MHI_HIP(hipGetLastError());
    }
    ++passes;
    MHI_HIP(hipMemcpyAsync(counts.data(), d_counts, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    MHI_HIP(hipStreamSynchronize(ctx->stream)); // (also: `tiles` and `st` may change now)
    retry.clear();
    for (uint32_t j : active) {
      const u128 tau = (u128)st[j].tau;
      const unsigned long long count = counts[j];
      u128 nt;
      if (count > st[j].limit) { // too many: lower tau, aiming at a quarter of the capacity
        hi[j] = tau;
        nt = tau * (u128)std::max<uint64_t>(st[j].limit / 2, 1) / (u128)count;
        if (nt <= lo[j] || nt >= hi[j]) nt = lo[j] + (hi[j] - lo[j]) / 2;
      } else if (count < s && tau < TOP) { // too few: raise tau, aiming at 4 s
        lo[j] = tau;
        nt = count ? tau * (u128)(4 * (uint64_t)s) / (u128)count : tau * 16;
        if (nt > TOP) nt = TOP;
        if (nt <= lo[j] || nt >= hi[j]) nt = lo[j] + (hi[j] - lo[j]) / 2;
      } else {
        continue;
      }
      if (nt <= lo[j] || nt >= hi[j] || passes >= 256) { // cannot happen while the count steps by one; never loop on it
        release();
        return fail(ctx, NTS_ERANGE, "nts_minhash_intervals: the threshold bracket of an interval closed without a sketch");
      }
      st[j].tau = (uint64_t)nt;
      retry.push_back(j);
    }
    active = retry;
    if (!active.empty()) {
      MHI_HIP(hipMemcpyAsync(d_retry, active.data(), active.size() * 4, hipMemcpyHostToDevice, ctx->stream));
      NTS_LAUNCH(k_mhi_reset, dim3((uint32_t)active.size() * MHI_SUB), dim3(256), 0, ctx->stream, d_retry, d_state, d_slots, d_counts);
      MHI_HIP(hipGetLastError());
      MHI_HIP(hipStreamSynchronize(ctx->stream)); // (`active` is rebuilt by the next turn)
    }
  }
  *passes_out = passes;
  // ---- the settled sets -> per interval the min(s, count) smallest, ascending
  std::vector<uint64_t> off(n + 1, 0), take(n + 1, 0);
  for (uint32_t j = 0; j < n; ++j) {
    off[j + 1] = off[j] + counts[j];
    take[j + 1] = take[j] + std::min<uint64_t>(s, counts[j]);
    n_out[i0 + j] = (uint32_t)std::min<uint64_t>(s, counts[j]);
  }
  const uint64_t total = off[n], total_take = take[n];
  if (total == 0) {
    release();
    return NTS_OK;
  }
  if (total > 0xFFFFFFFFull) {
    release();
    return fail(ctx, NTS_ERANGE, "nts_minhash_intervals: too many survivors in one chunk");
  }
  MHI_HIP(dev_malloc((void**)&d_list, total * 8));
  MHI_HIP(dev_malloc((void**)&d_sorted, total * 8));
  MHI_HIP(dev_malloc((void**)&d_take, total_take * 8));
  uint64_t *d_off = nullptr, *d_take_off = nullptr;
  MHI_RC(ws_upload(ctx, "mhi_off", off, &d_off));
  MHI_RC(ws_upload(ctx, "mhi_take_off", take, &d_take_off));
  MHI_HIP(hipMemsetAsync(d_counts, 0, (size_t)n * 8, ctx->stream)); // (the counts are on the host: the array serves as the cursors)
  NTS_LAUNCH(k_mhi_compact, dim3(n * MHI_SUB), dim3(256), 0, ctx->stream, d_state, d_slots, d_off, d_counts, d_list);
  MHI_HIP(hipGetLastError());
  size_t tmp_bytes = 0;
  MHI_HIP(rocprim::segmented_radix_sort_keys(nullptr, tmp_bytes, d_list, d_sorted, (unsigned int)total, n, d_off, d_off + 1, 0, 64, ctx->stream));
  MHI_HIP(dev_malloc(&d_tmp, std::max<size_t>(tmp_bytes, 16)));
  MHI_HIP(rocprim::segmented_radix_sort_keys(d_tmp, tmp_bytes, d_list, d_sorted, (unsigned int)total, n, d_off, d_off + 1, 0, 64, ctx->stream));
  NTS_LAUNCH(k_mhi_take, dim3(n * MHI_SUB), dim3(256), 0, ctx->stream, d_sorted, d_off, d_take_off, d_take);
  MHI_HIP(hipGetLastError());
  std::vector<uint64_t> host(total_take);
  MHI_HIP(hipMemcpyAsync(host.data(), d_take, total_take * 8, hipMemcpyDeviceToHost, ctx->stream));
  MHI_HIP(hipStreamSynchronize(ctx->stream));
  release();
#undef MHI_HIP
#undef MHI_RC
  for (uint32_t j = 0; j < n; ++j)
    if (take[j + 1] > take[j]) memcpy(out + (i0 + j) * (uint64_t)s, host.data() + take[j], (take[j + 1] - take[j]) * 8);
  return NTS_OK;
}

int minhash_intervals_run(nts_ctx* ctx, const nts_genome* g, uint32_t k, uint32_t s, const nts_interval* iv, uint64_t n_iv, uint64_t* out,
                          uint32_t* n_out, uint64_t* n_kmers)
{
  ctx->last_mhi_passes = ctx->last_mhi_chunks = 0;
  ctx->last_mhi_sweeps = 0;
  if (n_iv == 0) return NTS_OK;
  // ---- the intervals against the stretches of valid bases: runs of k-mers that lie wholly inside an interval
  std::vector<IvPiece> pieces;
  std::vector<uint64_t> piece_at, nk, caps(n_iv, 0);
  {
    const int rc = iv_cut_pieces(ctx, g, k, iv, n_iv, "nts_minhash_intervals", pieces, piece_at, nk);
    if (rc) return rc;
  }
  uint64_t knob_cap = 0;
  if (const char* v = NTS_KNOB("NTS_MINHASH_CAP")) knob_cap = strtoull(v, nullptr, 0);
  for (uint64_t i = 0; i < n_iv; ++i) {
    if (n_kmers) n_kmers[i] = nk[i];
    n_out[i] = 0;
    uint64_t cap = std::max<uint64_t>(64, std::min<uint64_t>(nk[i] > ((uint64_t)1 << 60) ? ~0ull : 4 * nk[i], (uint64_t)16 * s));
    if (knob_cap) cap = std::max<uint64_t>(knob_cap, (uint64_t)4 * s);
    caps[i] = mh_pow2_at_least(cap);
  }
  uint64_t budget = (uint64_t)2 << 30;
  if (const char* v = NTS_KNOB("NTS_MINHASH_IV_BUDGET")) budget = std::max<uint64_t>(strtoull(v, nullptr, 0), 1);
  HashParams hp;
  {
    const int rc = hash_params_for(ctx, k, &hp);
    if (rc) return rc;
  }
  constexpr uint64_t MAX_CHUNK = (uint64_t)1 << 20; // intervals per chunk: the small kernels launch MHI_SUB workgroups for each
  for (uint64_t i0 = 0; i0 < n_iv;) {
    uint64_t i1 = i0, bytes = 0;
    while (i1 < n_iv && i1 - i0 < MAX_CHUNK && (i1 == i0 || bytes + caps[i1] * 8 <= budget)) bytes += caps[i1++] * 8;
    uint32_t passes = 0;
    const int rc = minhash_intervals_chunk(ctx, g, hp, s, i0, i1, pieces, piece_at, nk, caps, out, n_out, &passes);
    if (rc) return rc;
    ctx->last_mhi_passes = std::max(ctx->last_mhi_passes, passes);
    ctx->last_mhi_sweeps += passes;
    ctx->last_mhi_chunks += 1;
    i0 = i1;
  }
  return NTS_OK;
}

// ---- pair counts of bottom-s sketches (nts_minhash_pairs) -----------------------------------------------------------------------
// One wave per pair.  A = sk[a], B = sk[b], both ascending and distinct.  Lane l of a turn takes A[i], i = 64 t + l: j = the number
// of B's elements below A[i] (binary search), m = whether B holds A[i] itself.  Its rank in the union is i + j - (common elements
// before it), the latter from a ballot and the turns before.  shared = common elements of rank below s; |bottom-s(A u B)| =
// min(s, |A| + |B| - common).
__global__ __launch_bounds__(256) void k_minhash_pairs(const uint64_t* __restrict__ sk, const uint32_t* __restrict__ n_sk, uint32_t s,
                                                       const uint64_t* __restrict__ pair_a, const uint64_t* __restrict__ pair_b, uint64_t n_pairs,
                                                       uint32_t* __restrict__ shared, uint32_t* __restrict__ usize)
{
  const uint64_t pair = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= n_pairs) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t ia = pair_a[pair], ib = pair_b[pair];
  const uint64_t* A = sk + ia * s;
  const uint64_t* B = sk + ib * s;
  const uint32_t na = n_sk[ia], nb = n_sk[ib];
  uint32_t common = 0, in_sketch = 0;
  for (uint32_t i0 = 0; i0 < na; i0 += 64) {
    const uint32_t i = i0 + lane;
    bool m = false;
    uint32_t j = 0;
    if (i < na) {
      const uint64_t x = A[i];
      uint32_t lo = 0, hi = nb; // first j with B[j] >= x
      while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (B[mid] < x)
          lo = mid + 1;
        else
          hi = mid;
      }
      j = lo;
      m = j < nb && B[j] == x;
    }
    const unsigned long long ball = __ballot(m);
    const uint32_t before = common + (uint32_t)__popcll(ball & ((1ull << lane) - 1ull));
    const bool inside = m && (uint64_t)i + j - before < s;
    in_sketch += (uint32_t)__popcll(__ballot(inside));
    common += (uint32_t)__popcll(ball);
  }
  if (lane == 0) {
    shared[pair] = in_sketch;
    usize[pair] = (uint32_t)min((uint64_t)s, (uint64_t)na + nb - common);
  }
}

int minhash_pairs_run(nts_ctx* ctx, uint32_t s, const uint64_t* sk, const uint32_t* n_sk, uint64_t n_sketches, const uint64_t* pair_a,
                      const uint64_t* pair_b, uint64_t n_pairs, uint32_t* shared, uint32_t* usize)
{
  if (n_pairs == 0) return NTS_OK;
  for (uint64_t i = 0; i < n_sketches; ++i)
    if (n_sk[i] > s) return fail(ctx, NTS_EINVAL, "nts_minhash_pairs: a sketch longer than s");
  for (uint64_t p = 0; p < n_pairs; ++p)
    if (pair_a[p] >= n_sketches || pair_b[p] >= n_sketches) return fail(ctx, NTS_EINVAL, "nts_minhash_pairs: sketch index out of range");
  if ((n_pairs + 3) / 4 > 0xFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_minhash_pairs: too many pairs for one call");
  uint64_t *d_sk = nullptr, *d_pairs = nullptr;
  uint32_t *d_n = nullptr, *d_res = nullptr;
  auto release = [&]() {
    hipStreamSynchronize(ctx->stream);
    dev_free(d_sk);
    dev_free(d_pairs);
    dev_free(d_n);
    dev_free(d_res);
  };
  hipError_t e = dev_malloc((void**)&d_sk, n_sketches * s * 8);
  if (e == hipSuccess) e = dev_malloc((void**)&d_pairs, n_pairs * 16);
  if (e == hipSuccess) e = dev_malloc((void**)&d_n, n_sketches * 4);
  if (e == hipSuccess) e = dev_malloc((void**)&d_res, n_pairs * 8);
  if (e == hipSuccess) e = hipMemcpyAsync(d_sk, sk, n_sketches * s * 8, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_n, n_sk, n_sketches * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_pairs, pair_a, n_pairs * 8, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_pairs + n_pairs, pair_b, n_pairs * 8, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    ScopedTimer t(ctx, "minhash_pairs", true);
    NTS_LAUNCH(k_minhash_pairs, dim3((uint32_t)((n_pairs + 3) / 4)), dim3(256), 0, ctx->stream, d_sk, d_n, s, d_pairs, d_pairs + n_pairs, n_pairs,
               d_res, d_res + n_pairs);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(shared, d_res, n_pairs * 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(usize, d_res + n_pairs, n_pairs * 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  release();
  HIP_TRY(ctx, e);
  return NTS_OK;
}

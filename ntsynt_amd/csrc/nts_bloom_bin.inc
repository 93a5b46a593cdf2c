// Binned Bloom-filter build (row A2 at scale).  Included inside the anonymous namespace of ntsynt_hip.hip.
//
// One atomic OR per k-mer tops out at ~27 G/s on this chip whatever the size of the target (scripts/atomic_rate.py:
// the atomic units, not HBM, are the limit), i.e. ~0.15 s for a human-scale genome.  The build below replaces the
// global atomics by streaming passes:
//
//   k_bin1  hash every k-mer (bases from the 2-bit image, rolling as in k_hash_select), bit index idx = h0 mod bits; partition by the top
//           bits of idx into B1 <= 512 level-1 buckets.  A workgroup sorts its 8192 indices by bucket in LDS, reserves
//           room in each bucket with one returning atomic per (workgroup, bucket) and writes runs of 32-bit residues.
//   k_bin2  (only when there are more than 512 final buckets) the same partition step inside every level-1 bucket,
//           by the next log2(B2) <= 9 bits.
//   k_bin3  one workgroup per final bucket = 2^19 filter bits: a 64 KiB LDS bitmap (two workgroups per CU: one loads its
//           residues while the other streams its bitmap out; 128 KiB buckets left one workgroup per CU and took 0.39
//           instead of 0.27 ms per 100 Mbp) takes the bucket's residues with
//           LDS atomics and is then OR-ed into the filter with plain 16-byte loads and stores (the words of a final
//           bucket belong to exactly one workgroup).
//
// Buckets have fixed capacities (mean + slack; hashes are uniform, but a repeat family puts all its copies into one
// bucket): an index that does not fit is OR-ed into the filter directly with an atomic, so the result never
// depends on the capacities.  (Only k-mers longer than 128 bases take the direct path for every index.)  Traffic: ~27 B per k-mer, all of it streaming.

constexpr uint32_t BIN_FINAL_SHIFT = 19;                 // 2^19 bits = 64 KiB of filter per final bucket (two workgroups of k_bin3 per CU)
constexpr uint32_t BIN_FINAL_WORDS = 1u << (BIN_FINAL_SHIFT - 5);
constexpr uint32_t BIN_MAX_B1 = 512;   // level-1 buckets (LDS: two 32-bit tables of this size next to the 48 KiB of sort staging)
constexpr uint32_t BIN_MAX_LOG2_B2 = 9;
constexpr uint32_t BIN3_THREADS = 1024;
constexpr uint32_t BIN_CNT_STRIDE = 32;                  // level-1 counters: one per 128-byte line
constexpr uint32_t BIN_THREADS = 512;                    // k_bin2: 8192 indices per workgroup, 16 per lane
constexpr uint32_t BIN_PER = KEY_TILE / BIN_THREADS;
static_assert((1u << BIN_MAX_LOG2_B2) <= BIN_THREADS, "k_bin2 clears and scans its level-2 counters with one lane per counter");
#if defined(NTS_EXPERIMENTS) && defined(NTS_BIN1_THREADS)
constexpr uint32_t BIN1_THREADS = NTS_BIN1_THREADS;      // (measurement only: 512 = sixteen k-mers per lane, four waves per SIMD)
#else
constexpr uint32_t BIN1_THREADS = 1024;                  // k_bin1: 8 per lane (its 76 KB of LDS allow two workgroups per CU:
#endif
constexpr uint32_t BIN1_PER = KEY_TILE / BIN1_THREADS;   // only a wide workgroup fills the SIMDs)
constexpr uint32_t BIN1_SIDE = 48 * 8 / BIN1_PER;        // lanes per tile whose k-mers span a run boundary (3 KB of LDS)
constexpr uint32_t BIN1_PAIR_MASK = BIN1_PER >= 16 ? 0x33333333u : 0x3333u; // (incoming, outgoing) pairs of a lane's steps, four bits each
static_assert(BIN1_PER == 8 || BIN1_PER == 16, "a lane's outgoing and incoming bases are one 32-bit word each");

int ensure_pack(nts_ctx* ctx, const nts_genome* g); // (defined with the pruned sketch, further down)

// Indices that do not go through the buckets (a bucket that is full: the copies of a repeat; tiles in pieces) are set in the
// filter directly.  When the filter was empty before the build, k_bin3 stores its bitmaps without reading the filter first
// (a third of its traffic), so such indices are parked in a list and set after it (k_bin_late); a list that runs full falls
// back to setting them at once and raises `dirty`, which makes k_bin3 read and OR as it does for a filter with content.
//
// AND build (nts_bf_insert_and: acc &= the genome's filter, the cascade level of src/ntsynt_make_common_bf.cpp:134-160 fused into
// the build's last pass): k_bin3 ANDs the running filter's slice with its bitmap, so a bit that bypassed the buckets would be
// lost there.  Such an index looks at the running filter -- still untouched while k_bin1 / k_bin2 run -- and only matters if its
// bit is set; the first k-mer to find it set takes the bit out with a returning atomic (so the copies of a repeat park ONE
// entry per bit, not one per copy) and parks the index; k_bin_late puts the parked bits back once k_bin3 is through.  A list that
// runs full puts its bit back at once and raises `dirty`: k_bin3 then leaves the filter alone, k_bin_late restores the parked
// bits -- the running filter is exactly what it was -- and the host redoes the level with a filter of the genome's own.
struct BinLate
{
  uint64_t* list;            // nullptr: set directly
  unsigned long long* count; // indices that bypassed the buckets (entries asked for: may exceed cap)
  uint64_t cap;
  uint32_t* dirty;
  uint32_t and_mode;
};

// A slot of the list for every lane that is here (the lanes of a wave that took the same branch): one returning atomic per wave, not
// per lane.  On an assembly-like genome two k-mers in a hundred bypass their buckets -- 58 M per 3 Gbp, the copies of satellite units
// and young repeats and whatever shares a final bucket with them -- and 58 M additions to ONE address took 90 ms (a whole build: 20).
__device__ __forceinline__ unsigned long long bin_late_slot(unsigned long long* count)
{
  const unsigned long long here = __ballot(1);
  const uint32_t lane = __lane_id();
  const uint32_t leader = (uint32_t)__ffsll((long long)here) - 1u;
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd(count, (unsigned long long)__popcll(here));
  base = __shfl(base, (int)leader, 64);
  return base + (unsigned long long)__popcll(here & ((1ULL << lane) - 1ULL));
}

__device__ __forceinline__ void bin_set_late(const BinLate& L, uint32_t* bf, uint64_t idx)
{
  if (L.and_mode) {
    uint32_t* w = &bf[idx >> 5];
    const uint32_t bit = 1u << (idx & 31);
    if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) return; // not in the running filter: the AND drops it anyway
    if (!(atomicAnd(w, ~bit) & bit)) return;                                             // another copy of this k-mer parked it already
    const unsigned long long s = bin_late_slot(L.count);
    if (s < L.cap) {
      L.list[s] = idx;
      return;
    }
    atomicOr(w, bit);
    atomicOr(L.dirty, 1u);
    return;
  }
  const unsigned long long s = bin_late_slot(L.count);
  if (L.list) {
    if (s < L.cap) {
      L.list[s] = idx;
      return;
    }
    atomicOr(L.dirty, 1u);
  }
  bf_set_unless_set(bf, idx);
}

struct BinParams
{
  const uint8_t* code;
  const uint32_t* pack; // the bases 2 bits each, 16 per word (nts_genome::d_pack)
  const uint64_t* run_pos;
  const uint64_t* run_vstart;
  uint32_t n_runs;
  uint64_t n_valid;
  HashParams hp;
  FastMod fm;
  uint32_t* bf;     // filter words
  uint32_t sh1;     // idx >> sh1 = level-1 bucket, idx & (2^sh1 - 1) = residue
  uint32_t B1;
  uint32_t* cnt1;   // [B1 * BIN_CNT_STRIDE] elements reserved so far, one counter per 128-byte line: every workgroup adds to
                    // every counter, and counters sharing a line are served one after the other by one L2 channel
  uint32_t* out1;   // [B1][cap1] residues
  uint32_t cap1;
  uint32_t idx32;   // B1 * cap1 < 2^32: a residue's place in out1 is a 32-bit index
  BinLate late;
};

// Exclusive scan of s_cnt[0 .. n) in place (n <= 2 * BIN_THREADS, every lane of the workgroup takes part), with
// got[q] = reserve(b, count) called once per non-empty bucket b = 2 * tid + q before its count is replaced by the
// offset.  The caller stores got[] (s_gbase[b]) only after its LDS scatter, so that the round trip of the returning
// global atomic inside reserve() overlaps the scan and the scatter instead of stalling the workgroup at once.
template <typename Reserve>
__device__ __forceinline__ void bin_scan(uint32_t* s_cnt, uint32_t* s_wave, uint32_t n, Reserve&& reserve, uint32_t (&got)[2], uint32_t (&excl)[2],
                                         uint32_t tid = threadIdx.x, uint32_t* cnt_out = nullptr)
{
  uint32_t c[2], sum = 0;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const uint32_t b = 2u * tid + q;
    c[q] = b < n ? s_cnt[b] : 0u;
    got[q] = 0;
    if (c[q]) got[q] = reserve(b, c[q]);
    sum += c[q];
  }
  // inclusive scan of `sum` over the wave, then over the waves
  uint32_t inc = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(inc, d, 64);
    if ((int)(tid & 63u) >= d) inc += up;
  }
  if ((tid & 63u) == 63u) s_wave[tid >> 6] = inc;
  __syncthreads();
  uint32_t before = inc - sum;
  for (uint32_t wv = 0; wv < (tid >> 6); ++wv) before += s_wave[wv];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const uint32_t b = 2u * tid + q;
    if (b < n) s_cnt[b] = before;
    excl[q] = before;
    if (cnt_out && b < n) cnt_out[b] = c[q]; // (the counts, parked where the caller will read them back: not a register each across its scatter)
    before += c[q];
  }
  __syncthreads();
}

template <typename Reserve>
__device__ __forceinline__ void bin_scan(uint32_t* s_cnt, uint32_t* s_wave, uint32_t n, Reserve&& reserve, uint32_t (&got)[2])
{
  uint32_t excl[2];
  bin_scan(s_cnt, s_wave, n, reserve, got, excl);
}

// First k-mer of a lane from an LDS table, two bases per read: tab2[g * 16 + v] = init[2g][v & 3] ^ init[2g + 1][v >> 2] (the second
// term only while 2g + 1 < k), `bases` = the k-mer 2 bits per base.  The table the other kernels use (four bases per read,
// [ceil(k/4)][256] entries in device memory) would put vector-memory reads between the loads of a tile's bases and its hashing --
// reads that queue behind the stores of the tile before (k_bin1).
constexpr uint32_t BIN1_INIT_GROUPS = 32; // k <= 64 (8 KB of LDS; two workgroups of k_bin1 just fit a CU)
__device__ __forceinline__ void hash_init_lds(const ulonglong2* tab2, uint32_t k, const uint32_t (&bases)[4], uint64_t& f, uint64_t& r)
{
  f = 0;
  r = 0;
  const uint32_t ng = (k + 1u) >> 1;
#pragma unroll
  for (uint32_t g0 = 0; g0 < BIN1_INIT_GROUPS; g0 += 4) {
    if (g0 >= ng) break;
    ulonglong2 e[4]; // (the rows from ceil(k/2) on hold zeros: nothing is predicated)
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      const uint32_t g = g0 + q;
      e[q] = tab2[g * 16u + ((bases[g >> 3] >> (4u * (g & 7u))) & 15u)];
    }
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      f ^= e[q].x;
      r ^= e[q].y;
    }
  }
}

// The same with THREE bases per read for k <= 24 (the reference's default k): tab3[g * 64 + v] = init[3g][v & 3] ^ init[3g + 1][(v >> 2) & 3]
// ^ init[3g + 2][v >> 4] (terms past k left out) -- eight reads instead of twelve at k = 24, in the same 8 KB.
constexpr uint32_t BIN1_INIT3_K = 24;
__device__ __forceinline__ void hash_init_lds3(const ulonglong2* tab3, const uint32_t (&bases)[4], uint64_t& f, uint64_t& r)
{
  f = 0;
  r = 0;
  ulonglong2 e[8]; // (rows past ceil(k/3) hold zeros)
#pragma unroll
  for (uint32_t g = 0; g < 8; ++g) {
    const uint32_t bit = 6u * g, wd = bit >> 5, sh = bit & 31u;
    const uint32_t six = (sh <= 26u ? bases[wd] >> sh : __builtin_amdgcn_alignbit(bases[wd + 1], bases[wd], sh)) & 63u;
    e[g] = tab3[g * 64u + six];
  }
#pragma unroll
  for (uint32_t g = 0; g < 8; ++g) {
    f ^= e[g].x;
    r ^= e[g].y;
  }
}

// a uniform 64-bit word through the scalar cache (read-only tables)
__device__ __forceinline__ uint64_t bin_sload64(const uint64_t* p)
{
  uint64_t v;
  asm volatile("s_load_dwordx2 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(p) : "memory");
  return v;
}

// very long k-mers (k > FAST_K_MAX): walk the run table, OR directly
__global__ __launch_bounds__(BIN1_THREADS) void k_bin1_long(BinParams P)
{
  __shared__ uint64_t s_tab[36];
  const uint32_t tid = threadIdx.x;
  if (tid < 16) {
    s_tab[tid] = P.hp.roll_f[tid];
    s_tab[16 + tid] = P.hp.roll_r[tid];
  }
  if (tid < 4) s_tab[32 + tid] = P.hp.seed[tid];
  __syncthreads();
  const uint32_t k = P.hp.k;
  const uint64_t J0 = (uint64_t)blockIdx.x * KEY_TILE;
  uint64_t j = J0 + (uint64_t)BIN1_PER * tid;
  if (j >= P.n_valid) return;
  const uint64_t j_end = min(j + (uint64_t)BIN1_PER, min(P.n_valid, J0 + KEY_TILE));
  uint32_t lo = 0, hi = P.n_runs;
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (P.run_vstart[mid] <= j)
      lo = mid;
    else
      hi = mid;
  }
  uint32_t ri = lo;
  while (j < j_end) {
    const uint64_t rv0 = P.run_vstart[ri], rv1 = P.run_vstart[ri + 1];
    const uint64_t seg_end = min(j_end, rv1);
    uint64_t p = P.run_pos[ri] + (j - rv0);
    uint64_t f = 0, r = 0;
    for (uint32_t i = 0; i < k; ++i) {
      f = srol1(f) ^ s_tab[32 + P.code[p + i]];
      r = srol1(r) ^ s_tab[32 + 3 - P.code[p + k - 1 - i]];
    }
    for (;;) {
      bf_set(P.bf, P.fm(f + r)); // (the host never asks for the store-only finish with k-mers this long)
      ++j;
      if (j >= seg_end) break;
      const uint32_t cout = P.code[p], cin = P.code[p + k];
      f = srol1(f) ^ s_tab[cin * 4 + cout];
      r = sror1(r ^ s_tab[16 + cin * 4 + cout]);
      ++p;
    }
    ++ri;
  }
}

// Persistent workgroups (two per CU), tiles taken round robin.  A tile's residues are written out while the NEXT tile is being
// hashed: a workgroup that ended with its stores kept its LDS and wave slots until the last store was acknowledged, and with two
// workgroups per CU that drain -- 3.6 of the kernel's 11.3 ms per 3 Gbp -- added to the hashing instead of hiding behind it.  Order
// inside a turn: the loads of this tile's bases, THEN the stores of the tile before (vector-memory operations of a wave retire in
// order: the loads are not held up by the stores behind them), then hashing -- which touches no vector memory (roll tables and
// the first-k-mer table sit in LDS) until the returning atomics of the scan, by when the stores have long drained.
template <int FM_FORM> // (FastMod::mod<FM_FORM>: the form of `h mod bits` fixed at compile time)
__global__ __launch_bounds__(BIN1_THREADS, BIN1_THREADS / 128) void k_bin1(BinParams P) // (two workgroups per CU: 64 registers)
{
  __shared__ uint64_t s_tab[36];
  __shared__ uint32_t s_cnt[BIN_MAX_B1];    // per-bucket counts, then exclusive offsets inside the tile
  __shared__ uint32_t s_gbase[BIN_MAX_B1];  // where the tile's run starts inside the global bucket, less where it starts in the tile
  __shared__ uint32_t s_wave[BIN1_THREADS / 64];
  __shared__ uint2 s_val[KEY_TILE];         // (residue, bucket), sorted by bucket: one scattered LDS write per k-mer instead of two (the
                                            // kernel's LDS pipe is busy all the time, half of it with bank conflicts of such writes)
  __shared__ uint64_t s_side[BIN1_SIDE * BIN1_PER]; // hashes of lanes with a run boundary inside
  __shared__ uint32_t s_nside[2];           // (by the parity of the turn: the tile before is still being written out)
  __shared__ uint32_t s_direct[2];          // k-mers of the tile that did not go through the sort (set directly)
  __shared__ uint32_t s_over[2];            // some bucket's reservation of the tile ran past its capacity (the write-out then checks every element)
  const bool idx32 = P.idx32 != 0;          // (round 5, A/B in one process, scripts/bloom_ab.py: insert -0.6 .. -2.5 %, AND level -1.3 .. -3.3 %)
  __shared__ ulonglong2 s_init2[BIN1_INIT_GROUPS * 16];
  __shared__ ulonglong2 s_roll2[16]; // {forward, reverse} roll-table entry of an (incoming, outgoing) pair: one 16-byte read per step
  const uint32_t tid = threadIdx.x;
  if (tid < 16) {
    s_tab[tid] = P.hp.roll_f[tid];
    s_tab[16 + tid] = P.hp.roll_r[tid];
    s_roll2[tid] = make_ulonglong2(P.hp.roll_f[tid], P.hp.roll_r[tid]);
  }
  if (tid < 4) s_tab[32 + tid] = P.hp.seed[tid];
  const uint32_t k = P.hp.k;
  const bool init3 = k <= BIN1_INIT3_K; // (round 5, A/B in one process: insert -2.0 %, AND level -5.4 %)
  if (init3 && tid < 8u * 64u) {
    const ulonglong2* tab = reinterpret_cast<const ulonglong2*>(P.hp.init);
    const uint32_t g = tid >> 6, v = tid & 63u;
    ulonglong2 e = make_ulonglong2(0, 0);
    for (uint32_t j = 0; j < 3; ++j)
      if (3u * g + j < k) {
        const ulonglong2 e2 = tab[(3u * g + j) * 4u + ((v >> (2u * j)) & 3u)];
        e.x ^= e2.x;
        e.y ^= e2.y;
      }
    s_init2[tid] = e;
  } else if (!init3 && tid < BIN1_INIT_GROUPS * 16u) {
    const ulonglong2* tab = reinterpret_cast<const ulonglong2*>(P.hp.init);
    const uint32_t g = tid >> 4, v = tid & 15u;
    ulonglong2 e = make_ulonglong2(0, 0);
    if (2u * g < k && k <= 2u * BIN1_INIT_GROUPS) {
      e = tab[(2u * g) * 4u + (v & 3u)];
      if (2u * g + 1u < k) {
        const ulonglong2 e2 = tab[(2u * g + 1u) * 4u + (v >> 2)];
        e.x ^= e2.x;
        e.y ^= e2.y;
      }
    }
    s_init2[tid] = e;
  }
  auto base_abs = [&](uint64_t p) -> uint32_t { return (P.pack[p >> 4] >> (2u * ((uint32_t)p & 15u))) & 3u; };
  uint32_t turn = 0;
  uint32_t tid_now = threadIdx.x; // (made opaque in every turn: offsets derived from it are not worth a register each across the loop)
  // the sorted tile in LDS -> the global buckets (n_sorted of its KEY_TILE slots are taken)
  auto write_out = [&](uint32_t n_sorted, uint32_t par_w) {
    if (idx32 && n_sorted == KEY_TILE && !s_over[par_w]) {
      // every reservation of the tile fitted its bucket (known since the scan) and out1 holds fewer than 2^32 residues: s_gbase is the
      // residue's place in out1 less its place in the tile -- no capacity test, no 64-bit product per element
      constexpr int HALF = (int)BIN1_PER / 2;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        uint2 e[HALF];
        uint32_t at[HALF];
#pragma unroll
        for (int u = 0; u < HALF; ++u) e[u] = s_val[(uint32_t)(h * HALF + u) * BIN1_THREADS + tid_now];
#pragma unroll
        for (int u = 0; u < HALF; ++u) at[u] = s_gbase[e[u].y] + ((uint32_t)(h * HALF + u) * BIN1_THREADS + tid_now);
#pragma unroll
        for (int u = 0; u < HALF; ++u) P.out1[at[u]] = e[u].x;
      }
      return;
    }
    const uint32_t off32 = idx32 ? P.cap1 : 0u; // (s_gbase holds b * cap1 more than the place in the bucket)
    if (n_sorted == KEY_TILE) {
      // (uniform) nothing predicated: the LDS reads of the eight elements of a lane go out together, then the table reads, then the stores
      bool over = false;
      constexpr int HALF = (int)BIN1_PER / 2; // (four at a time: the registers of this tile's loaded bases are live as well)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        uint2 e[HALF];
        uint32_t pos[HALF];
#pragma unroll
        for (int u = 0; u < HALF; ++u) e[u] = s_val[(uint32_t)(h * HALF + u) * BIN1_THREADS + tid_now];
#pragma unroll
        for (int u = 0; u < HALF; ++u) pos[u] = s_gbase[e[u].y] - e[u].y * off32 + ((uint32_t)(h * HALF + u) * BIN1_THREADS + tid_now);
#pragma unroll
        for (int u = 0; u < HALF; ++u) {
          if (pos[u] < P.cap1) P.out1[(uint64_t)e[u].y * P.cap1 + pos[u]] = e[u].x;
          over |= pos[u] >= P.cap1;
        }
      }
      if (over) { // (rare: a full bucket -- the copies of a repeat; from LDS again, register arrays indexed by a loop counter would live in scratch)
        for (uint32_t i = tid_now; i < KEY_TILE; i += BIN1_THREADS) {
          const uint2 x = s_val[i];
          if (s_gbase[x.y] - x.y * off32 + i >= P.cap1) bin_set_late(P.late, P.bf, ((uint64_t)x.y << P.sh1) | x.x);
        }
      }
      return;
    }
    for (uint32_t i = tid_now; i < n_sorted; i += BIN1_THREADS) {
      const uint2 e = s_val[i];
      const uint32_t b = e.y;
      const uint32_t pos = s_gbase[b] - b * off32 + i;
      if (pos < P.cap1)
        P.out1[(uint64_t)b * P.cap1 + pos] = e.x;
      else
        bin_set_late(P.late, P.bf, ((uint64_t)b << P.sh1) | e.x);
    }
  };
  const uint32_t n_tiles = (uint32_t)((P.n_valid + KEY_TILE - 1) / KEY_TILE); // (the host checks that it fits)
  uint32_t lo = 0;                 // run of the current tile's first k-mer, its first and last compact index, its position
  uint64_t v0 = 0, v1 = 0, p0 = 0; // (v1 = 0: the first turn searches)
  uint32_t prev_sorted = 0; // elements of the tile before still to be written out
  bool pending = false;
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x, ++turn) {
    const uint32_t par = turn & 1u;
    asm volatile("" : "+v"(tid_now));
    const uint32_t tid = tid_now; // (shadows the kernel's: what is derived from it stays inside the turn)
    if (tid == 0) s_nside[par] = s_direct[par] = s_over[par] = 0;
    for (uint32_t b = tid; b < P.B1; b += BIN1_THREADS) s_cnt[b] = 0;
    const uint64_t J0 = (uint64_t)tile * KEY_TILE;
    const uint32_t tile_len = (uint32_t)min((uint64_t)KEY_TILE, P.n_valid - J0);
    // The run of the tile's first k-mer is carried from turn to turn (tiles only move forward): nearly always the same run, and then
    // nothing is read; else a galloping search from where the last one ended.  Scalar loads spelled out: the table is read-only,
    // but the compiler, seeing stores in the loop, reads uniform addresses through the vector path -- a dozen dependent round
    // trips per tile at the top of every turn.
    if (J0 >= v1) { // (uniform)
      uint32_t step = 1, hi = lo + 1;
      while (hi < P.n_runs && bin_sload64(P.run_vstart + hi) <= J0) {
        lo = hi;
        hi = min(P.n_runs, hi + step);
        step <<= 1;
      }
      while (hi - lo > 1) { // run_vstart[lo] <= J0 < run_vstart[hi] (run_vstart[n_runs] = n_valid > J0)
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (bin_sload64(P.run_vstart + mid) <= J0)
          lo = mid;
        else
          hi = mid;
      }
      v0 = bin_sload64(P.run_vstart + lo);
      v1 = bin_sload64(P.run_vstart + lo + 1);
      p0 = bin_sload64(P.run_pos + lo);
    }
    const bool single = J0 + tile_len <= v1;
    uint32_t run_end = lo + 1u; // one past the run of the tile's last k-mer (uniform, scalar loads)
    if (!single) {
      const uint64_t j_last = J0 + tile_len - 1u;
      uint32_t a = lo, b = (uint32_t)min((uint64_t)P.n_runs, (uint64_t)lo + tile_len);
      while (b - a > 1) {
        const uint32_t mid = a + ((b - a) >> 1);
        if (bin_sload64(P.run_vstart + mid) <= j_last)
          a = mid;
        else
          b = mid;
      }
      run_end = a + 1u;
    }
    __syncthreads();
    // ---- the lane's bases come from the 2-bit image of the genome, as in k_hash_select: eight outgoing and eight
    //      incoming bases in one register each, the first k-mer from a table ---------------------------------------
    const uint32_t first = BIN1_PER * tid;
    const uint32_t n_mine = first < tile_len ? min(BIN1_PER, tile_len - first) : 0u;
    uint64_t f = 0, r = 0;
    uint32_t even = 0, odd = 0; // (incoming, outgoing) base pairs of steps 0,2,4,6 and 1,3,5,7, four bits each
    // A tile of a fragmented assembly spans several runs (contig ends, N stretches): every lane looks up the run of its
    // first k-mer; a lane whose eight k-mers cross into another run hashes each of them from scratch (`apart`).
    const uint64_t j_lane = J0 + first;
    uint32_t run = lo;
    bool apart = false;
    uint64_t xo = 0;
    uint32_t ro[5] = { 0, 0, 0, 0, 0 }, ri2[2] = { 0, 0 };
    if (n_mine) {
      if (!single) {
        uint32_t rl = lo, rh = run_end; // (the runs this tile touches, not the table from `lo` to its end: k_hash_select_hi, same remark)
        while (rh - rl > 1) {
          const uint32_t mid = rl + ((rh - rl) >> 1);
          if (P.run_vstart[mid] <= j_lane)
            rl = mid;
          else
            rh = mid;
        }
        run = rl;
      }
      const uint64_t rv0 = single ? v0 : P.run_vstart[run], rv1 = single ? v1 : P.run_vstart[run + 1];
      apart = j_lane + n_mine > rv1;
      xo = (single ? p0 : P.run_pos[run]) + (j_lane - rv0);
      const uint32_t* wo = P.pack + (xo >> 4);
      const uint32_t* wi = P.pack + ((xo + k) >> 4);
      if (k <= 64) {
#pragma unroll
        for (int q = 0; q < 5; ++q) ro[q] = wo[q];
      } else {
        ro[0] = wo[0];
        ro[1] = wo[1];
      }
      ri2[0] = wi[0];
      ri2[1] = wi[1];
    }
    __builtin_amdgcn_sched_barrier(0); // (the loads above are issued before the stores below)
    if (pending) write_out(prev_sorted, par ^ 1u);
    __builtin_amdgcn_sched_barrier(0);
    if (n_mine) {
      const uint32_t sh_o = 2u * ((uint32_t)xo & 15u), sh_i = 2u * ((uint32_t)(xo + k) & 15u);
      uint32_t O[4];
      if (k <= 64) {
#pragma unroll
        for (int q = 0; q < 4; ++q) O[q] = __builtin_amdgcn_alignbit(ro[q + 1], ro[q], sh_o);
        if (init3)
          hash_init_lds3(s_init2, O, f, r);
        else
          hash_init_lds(s_init2, k, O, f, r);
      } else {
        O[0] = __builtin_amdgcn_alignbit(ro[1], ro[0], sh_o);
        hash_init(P.hp, [&](uint32_t i) { return base_abs(xo + i); }, f, r);
      }
      const uint32_t I0 = __builtin_amdgcn_alignbit(ri2[1], ri2[0], sh_i);
      even = (O[0] & BIN1_PAIR_MASK) | ((I0 & BIN1_PAIR_MASK) << 2);
      odd = ((O[0] >> 2) & BIN1_PAIR_MASK) | (I0 & (BIN1_PAIR_MASK << 2));
    }
    // a lane with a run boundary among its k-mers: each of them from scratch, parked in LDS for the unrolled loop below
    // (more such lanes than the side buffer holds -- runs of a few dozen k-mers -- set their bits directly)
    uint32_t side = 0, n_emit = n_mine;
    if (apart) {
      side = atomicAdd(&s_nside[par], 1u);
      for (uint32_t u = 0; u < n_mine; ++u) {
        const uint64_t j = j_lane + u;
        while (P.run_vstart[run + 1] <= j) ++run; // (j < n_valid = run_vstart[n_runs])
        const uint64_t s0 = P.run_pos[run] + (j - P.run_vstart[run]);
        uint64_t hf = 0, hr = 0; // (base by base: few registers, and it is the rare path)
        for (uint32_t i = 0; i < k; ++i) {
          hf = srol1(hf) ^ s_tab[32 + base_abs(s0 + i)];
          hr = srol1(hr) ^ s_tab[32 + 3 - base_abs(s0 + k - 1 - i)];
        }
        if (side < BIN1_SIDE)
          s_side[side * BIN1_PER + u] = hf + hr;
        else
          bin_set_late(P.late, P.bf, P.fm.template mod<FM_FORM>(hf + hr));
      }
      if (side >= BIN1_SIDE) {
        atomicAdd(&s_direct[par], n_mine);
        n_emit = 0;
        apart = false;
      }
    }
    // ---- hash, count per bucket; residue and (bucket, rank in the tile's bucket) stay in registers ------------------
    const uint64_t res_mask = (1ull << P.sh1) - 1ull;
    uint32_t res[BIN1_PER], pk[BIN1_PER];
    if (single && tile_len == KEY_TILE) {
      // (uniform) a whole tile inside one run -- all but a handful of the tiles of an assembly that is not in pieces: every lane
      // emits its eight k-mers, nothing is predicated
#pragma unroll
      for (int u = 0; u < (int)BIN1_PER; ++u) {
        const uint64_t idx = P.fm.template mod<FM_FORM>(f + r);
        const uint32_t pairs = (u & 1) ? odd : even;
        const int sh = 4 * (u >> 1) - 3;
        const uint32_t t8 = (sh < 0 ? pairs << 3 : pairs >> sh) & 0x78u; // 8 * (4 * incoming + outgoing)
        const ulonglong2 te = *reinterpret_cast<const ulonglong2*>(reinterpret_cast<const uint8_t*>(s_roll2) + 2u * t8);
        f = srol1(f) ^ te.x;
        r = sror1(r ^ te.y);
        const uint32_t b = (uint32_t)(idx >> P.sh1);
        res[u] = (uint32_t)(idx & res_mask);
        pk[u] = (b << 16) | atomicAdd(&s_cnt[b], 1u);
      }
    } else {
#pragma unroll
      for (int u = 0; u < (int)BIN1_PER; ++u) {
        uint64_t h = f + r;
        if (apart) h = s_side[side * BIN1_PER + (uint32_t)u]; // (rare: hashed from scratch above)
        const uint32_t pairs = (u & 1) ? odd : even;
        const int sh = 4 * (u >> 1) - 3;
        const uint32_t t8 = (sh < 0 ? pairs << 3 : pairs >> sh) & 0x78u; // 8 * (4 * incoming + outgoing)
        const ulonglong2 te = *reinterpret_cast<const ulonglong2*>(reinterpret_cast<const uint8_t*>(s_roll2) + 2u * t8);
        f = srol1(f) ^ te.x;
        r = sror1(r ^ te.y);
        pk[u] = 0xFFFFFFFFu;
        res[u] = 0;
        if ((uint32_t)u < n_emit) {
          const uint64_t idx = P.fm.template mod<FM_FORM>(h);
          const uint32_t b = (uint32_t)(idx >> P.sh1);
          res[u] = (uint32_t)(idx & res_mask);
          pk[u] = (b << 16) | atomicAdd(&s_cnt[b], 1u);
        }
      }
    }
    __syncthreads(); // (every lane is also through with the tile before: s_val and s_gbase are free)
    uint32_t got[2], excl[2];
    bin_scan(s_cnt, s_wave, P.B1, [&](uint32_t b, uint32_t count) { return atomicAdd(&P.cnt1[(uint64_t)b * BIN_CNT_STRIDE], count); }, got, excl, tid,
             idx32 ? s_gbase : nullptr);
    // ---- sort into LDS; the runs are written while the next tile is hashed --------------------------------------------
    if (single && tile_len == KEY_TILE) {
#pragma unroll
      for (int u = 0; u < (int)BIN1_PER; ++u) {
        const uint32_t b = pk[u] >> 16;
        const uint32_t sp = s_cnt[b] + (pk[u] & 0xFFFFu);
        s_val[sp] = make_uint2(res[u], b);
      }
    } else {
#pragma unroll
      for (int u = 0; u < (int)BIN1_PER; ++u) {
        if (pk[u] != 0xFFFFFFFFu) {
          const uint32_t b = pk[u] >> 16;
          const uint32_t sp = s_cnt[b] + (pk[u] & 0xFFFFu);
          s_val[sp] = make_uint2(res[u], b);
        }
      }
    }
    // position in the global bucket = s_gbase[b] + index in the sorted tile
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (2u * tid + q < P.B1) {
        const uint32_t cnt_b = idx32 ? s_gbase[2u * tid + q] : 0u; // (parked there by the scan)
        s_gbase[2u * tid + q] = got[q] - excl[q] + (idx32 ? (2u * tid + q) * P.cap1 : 0u);
        if (cnt_b && got[q] + cnt_b > P.cap1) s_over[par] = 1u; // (the returning atomic's answer is first looked at here, behind the scatter)
      }
    __syncthreads();
    prev_sorted = tile_len - s_direct[par];
    pending = true;
  }
  if (pending) write_out(prev_sorted, (turn + 1u) & 1u);
}

struct Bin2Params
{
  const uint32_t* cnt1; // [B1 * BIN_CNT_STRIDE]
  const uint32_t* in1;  // [B1][cap1]
  uint32_t cap1;
  uint32_t B1, tiles2; // level-1 buckets, tiles per level-1 bucket (the launch covers cap1)
  uint32_t log2_b2;
  uint32_t* cnt2;       // [B1 << log2_b2] packed words per level-2 bucket
  uint32_t* out2;       // [B1 << log2_b2][cap2] packed words (64 bits: three residues of BIN_FINAL_SHIFT bits and their valid bits)
  uint32_t cap2;        // words per level-2 bucket (even)
  uint32_t* bf;
  BinLate late;
};

// Level-2 buckets hold PACKED WORDS: three 19-bit residues per 64 bits (bits 0..56) and a "this one counts" bit for each (57..59).
// The second and third pass move 2.9 bytes per k-mer through this array instead of 4 each way.  A tile's run for a bucket is
// ceil(count / 3) words (the last one partly filled: valid bits say how much), reserved and written in words.
constexpr uint32_t BIN2_WORDS = ((KEY_TILE + 2u * (1u << BIN_MAX_LOG2_B2)) / 3u + 4u) & ~3u; // words of one tile, every bucket's last one partly filled

__device__ __forceinline__ void bin2_late_word(const Bin2Params& P, uint64_t fb, uint64_t w)
{
#pragma unroll
  for (uint32_t sub = 0; sub < 3; ++sub)
    if ((w >> (57u + sub)) & 1ull) bin_set_late(P.late, P.bf, (fb << BIN_FINAL_SHIFT) | ((w >> (19u * sub)) & ((1ull << BIN_FINAL_SHIFT) - 1ull)));
}

// A tile's trip through k_bin2.  FULL: all KEY_TILE residues are there (every tile of a bucket but its last) -- nothing is predicated,
// so the loads (16-byte ones: the order of the residues inside a bucket means nothing) and the LDS round trips of the scatter and
// the write-out go out in batches instead of one after the other (the predicated form compiled into sixteen global loads each
// followed by its own wait: 20 us per workgroup).
template <bool FULL>
__device__ __forceinline__ void bin2_tile(const Bin2Params& P, const uint32_t* __restrict__ in, uint32_t tile_len, uint32_t b1, uint32_t* s_cnt,
                                          uint32_t* s_tab, uint32_t* s_wdelta, uint32_t* s_wave, unsigned long long* s_words, uint16_t* s_wb)
{
  const uint32_t tid = threadIdx.x;
  const uint32_t B2 = 1u << P.log2_b2;
  // Counting first (LDS atomics that return nothing), slots afterwards from returning atomics on the scanned offsets: a rank per
  // element kept from the first pass to the second would be sixteen registers more, and the kernel wants eight waves per SIMD.
  uint32_t val[BIN_PER];
  if (FULL) {
    const uint4* in4 = reinterpret_cast<const uint4*>(in); // (bucket starts and tile starts are multiples of four entries)
#pragma unroll
    for (int q = 0; q < (int)BIN_PER / 4; ++q) {
      const uint4 v = in4[(uint32_t)q * BIN_THREADS + tid];
      val[4 * q] = v.x;
      val[4 * q + 1] = v.y;
      val[4 * q + 2] = v.z;
      val[4 * q + 3] = v.w;
    }
    // (all four loads before the first atomic: a statement that takes all sixteen values -- the optimiser otherwise sinks every
    // load to its first use, and a scheduling barrier comes too late to stop that)
    asm volatile("" : "+v"(val[0]), "+v"(val[1]), "+v"(val[2]), "+v"(val[3]), "+v"(val[4]), "+v"(val[5]), "+v"(val[6]), "+v"(val[7]),
                      "+v"(val[8]), "+v"(val[9]), "+v"(val[10]), "+v"(val[11]), "+v"(val[12]), "+v"(val[13]), "+v"(val[14]), "+v"(val[15]));
#pragma unroll
    for (int u = 0; u < (int)BIN_PER; ++u) atomicAdd(&s_cnt[val[u] >> BIN_FINAL_SHIFT], 1u);
  } else {
#pragma unroll
    for (int u = 0; u < (int)BIN_PER; ++u) { // (index clamped: the loads stay unconditional and go out together)
      const uint32_t e = (uint32_t)u * BIN_THREADS + tid;
      const uint32_t x = in[min(e, tile_len - 1u)];
      val[u] = e < tile_len ? x : 0xFFFFFFFFu; // level-1 residues have at most 28 bits
    }
    asm volatile("" : "+v"(val[0]), "+v"(val[1]), "+v"(val[2]), "+v"(val[3]), "+v"(val[4]), "+v"(val[5]), "+v"(val[6]), "+v"(val[7]),
                      "+v"(val[8]), "+v"(val[9]), "+v"(val[10]), "+v"(val[11]), "+v"(val[12]), "+v"(val[13]), "+v"(val[14]), "+v"(val[15]));
#pragma unroll
    for (int u = 0; u < (int)BIN_PER; ++u)
      if (val[u] != 0xFFFFFFFFu) atomicAdd(&s_cnt[val[u] >> BIN_FINAL_SHIFT], 1u);
  }
  // (only the sixteen values live on through the scan: left to itself the compiler also keeps their bucket numbers and LDS
  // addresses, forty-eight registers, spills, and goes back to one load at a time)
#pragma unroll
  for (int u = 0; u < (int)BIN_PER; ++u) asm volatile("" : "+v"(val[u]));
  __syncthreads();
  // ---- exclusive scan of (entries, words) per bucket, both in one 32-bit sum: entries in the low half (<= 8192), words in the
  //      high half (<= BIN2_WORDS); one returning global atomic per non-empty bucket reserves its words -----------------------------
  const uint64_t fb0 = (uint64_t)b1 << P.log2_b2;
  uint32_t c[2], got[2], sum = 0;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const uint32_t b = 2u * tid + q;
    const uint32_t n = b < B2 ? s_cnt[b] : 0u;
    const uint32_t nw = (n + 2u) / 3u;
    c[q] = n | (nw << 16);
    got[q] = 0;
    if (n) got[q] = atomicAdd(&P.cnt2[fb0 + b], nw);
    sum += c[q];
  }
  uint32_t inc = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(inc, d, 64);
    if ((int)(tid & 63u) >= d) inc += up;
  }
  if ((tid & 63u) == 63u) s_wave[tid >> 6] = inc;
  __syncthreads();
  uint32_t before = inc - sum, all = 0;
#pragma unroll
  for (uint32_t wv = 0; wv < BIN_THREADS / 64; ++wv) {
    const uint32_t t = s_wave[wv];
    if (wv < (tid >> 6)) before += t;
    all += t;
  }
  const uint32_t n_words = all >> 16; // words of this tile
  uint32_t woff[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const uint32_t b = 2u * tid + q;
    if (b < B2) {
      s_tab[b] = before;          // (first entry, first word) of the bucket inside the tile
      s_cnt[b] = before & 0xFFFFu; // the slots come from returning atomics on this
    }
    woff[q] = before >> 16;
    before += c[q];
  }
  __syncthreads();
  // ---- every residue into its third of its word (64-bit LDS atomics: the three residues of a word come from three lanes) --------
  constexpr int HALF = (int)BIN_PER / 4; // (batches of four: the sixteen values stay in registers next to them)
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    uint32_t slot[HALF], tab[HALF];
#pragma unroll
    for (int u = 0; u < HALF; ++u) {
      slot[u] = tab[u] = 0;
      if (FULL || val[h * HALF + u] != 0xFFFFFFFFu) {
        const uint32_t b = val[h * HALF + u] >> BIN_FINAL_SHIFT;
        slot[u] = atomicAdd(&s_cnt[b], 1u);
        tab[u] = s_tab[b];
      }
    }
#pragma unroll
    for (int u = 0; u < HALF; ++u)
      if (FULL || val[h * HALF + u] != 0xFFFFFFFFu) {
        const uint32_t r = slot[u] - (tab[u] & 0xFFFFu);  // rank inside the tile's run
        const uint32_t r3 = __umul24(r, 0xAAABu) >> 17;   // r / 3 (r < 2^15: a 24-bit multiply -- the compiler, not knowing the range,
        const uint32_t sub = r - 3u * r3;                 // took the quarter-rate 32-bit one, here and for 19 * sub)
        const uint32_t wi = (tab[u] >> 16) + r3;
        const uint64_t res = val[h * HALF + u] & ((1u << BIN_FINAL_SHIFT) - 1u);
        atomicOr(&s_words[wi], (unsigned long long)((res << __umul24(19u, sub)) | (1ull << (57u + sub))));
        if (sub == 0) s_wb[wi] = (uint16_t)(val[h * HALF + u] >> BIN_FINAL_SHIFT);
      }
  }
  // position of a word in its global bucket = s_wdelta[b] + its index in the tile
#pragma unroll
  for (int q = 0; q < 2; ++q)
    if (2u * tid + q < B2) s_wdelta[2u * tid + q] = got[q] - woff[q];
  __syncthreads();
  // ---- the words go out (the level-2 buckets of one level-1 bucket span less than 2^30 words: 32-bit offsets from a uniform base) --
  unsigned long long* const outb = reinterpret_cast<unsigned long long*>(P.out2) + fb0 * P.cap2;
  constexpr uint32_t WROUNDS = (BIN2_WORDS + BIN_THREADS - 1) / BIN_THREADS, WBATCH = 4;
  bool over = false;
#pragma unroll
  for (uint32_t u0 = 0; u0 < WROUNDS; u0 += WBATCH) {
    if (u0 * BIN_THREADS >= n_words) break; // (uniform)
    unsigned long long w[WBATCH];
    uint32_t wbk[WBATCH], pos[WBATCH];
#pragma unroll
    for (uint32_t u = 0; u < WBATCH; ++u) {
      const uint32_t i = min((u0 + u) * BIN_THREADS + tid, n_words - 1u); // (n_words >= 1: the tile is not empty)
      w[u] = s_words[i];
      wbk[u] = s_wb[i];
    }
#pragma unroll
    for (uint32_t u = 0; u < WBATCH; ++u) pos[u] = s_wdelta[wbk[u]] + ((u0 + u) * BIN_THREADS + tid);
#pragma unroll
    for (uint32_t u = 0; u < WBATCH; ++u) {
      const bool mine = (u0 + u) * BIN_THREADS + tid < n_words;
      const uint32_t at = wbk[u] * P.cap2 + pos[u];
      __builtin_assume(at < (1u << 30));
      if (mine && pos[u] < P.cap2) outb[at] = w[u];
      over |= mine && pos[u] >= P.cap2;
    }
  }
  // A full bucket (the copies of a repeat, and whatever shares a final bucket with them): its words bypass the buckets (BinLate).
  // Rare on an i.i.d. genome; on an assembly-like one two k-mers in a hundred end up here, spread thinly over two thirds of all tiles
  // (a final bucket that holds a satellite unit or a young repeat is full after a third of its level-1 bucket's tiles) -- a slot per
  // entry or per wave from the list's one counter made this kernel 44 ms instead of 5.  The workgroup reserves once: count (in the
  // AND build: after the look at the running filter, which clears the valid bits of the entries that do not matter), scan, one
  // atomic, write.  (From LDS again: register arrays indexed by a loop counter would live in scratch.)
  if (__syncthreads_or((int)over)) {
    constexpr uint64_t RM = (1ull << BIN_FINAL_SHIFT) - 1ull;
    uint32_t mine = 0;
    for (uint32_t i = tid; i < n_words; i += BIN_THREADS) {
      const uint32_t b = s_wb[i];
      if (s_wdelta[b] + i < P.cap2) continue;
      unsigned long long w = s_words[i];
      if (P.late.and_mode) {
#pragma unroll
        for (uint32_t sub = 0; sub < 3; ++sub)
          if ((w >> (57u + sub)) & 1ull) {
            const uint64_t idx = ((fb0 + b) << BIN_FINAL_SHIFT) | ((w >> (19u * sub)) & RM);
            uint32_t* wp = &P.bf[idx >> 5];
            const uint32_t bit = 1u << (idx & 31);
            const bool claimed = (__hip_atomic_load(wp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) && (atomicAnd(wp, ~bit) & bit);
            if (!claimed) w &= ~(1ull << (57u + sub));
          }
        s_words[i] = w;
      }
      mine += (uint32_t)__popcll((w >> 57) & 7ull);
    }
    uint32_t inc2 = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(inc2, d, 64);
      if ((int)(tid & 63u) >= d) inc2 += up;
    }
    if ((tid & 63u) == 63u) s_tab[tid >> 6] = inc2; // (s_tab has done its work)
    __syncthreads();
    uint32_t before2 = inc2 - mine, total = 0;
#pragma unroll
    for (uint32_t wv = 0; wv < BIN_THREADS / 64; ++wv) {
      const uint32_t t = s_tab[wv];
      if (wv < (tid >> 6)) before2 += t;
      total += t;
    }
    __syncthreads();
    if (tid == 0 && total) {
      const unsigned long long base = atomicAdd(P.late.count, (unsigned long long)total);
      s_tab[0] = (uint32_t)base;
      s_tab[1] = (uint32_t)(base >> 32);
    }
    __syncthreads();
    if (total) {
      unsigned long long at = (((unsigned long long)s_tab[1] << 32) | s_tab[0]) + before2;
      for (uint32_t i = tid; i < n_words; i += BIN_THREADS) {
        const uint32_t b = s_wb[i];
        if (s_wdelta[b] + i < P.cap2) continue;
        const unsigned long long w = s_words[i];
#pragma unroll
        for (uint32_t sub = 0; sub < 3; ++sub)
          if ((w >> (57u + sub)) & 1ull) {
            const uint64_t idx = ((fb0 + b) << BIN_FINAL_SHIFT) | ((w >> (19u * sub)) & RM);
            if (P.late.list && at < P.late.cap)
              P.late.list[at] = idx;
            else if (P.late.and_mode) { // no room: the bit goes back, the level is redone the plain way
              atomicOr(&P.bf[idx >> 5], 1u << (idx & 31));
              atomicOr(P.late.dirty, 1u);
            } else {
              if (P.late.list) atomicOr(P.late.dirty, 1u);
              bf_set_unless_set(P.bf, idx);
            }
            ++at;
          }
      }
    }
  }
}

__global__ __launch_bounds__(BIN_THREADS, 8) void k_bin2(Bin2Params P)
{
  __shared__ uint32_t s_cnt[1u << BIN_MAX_LOG2_B2];
  __shared__ uint32_t s_tab[1u << BIN_MAX_LOG2_B2];
  __shared__ uint32_t s_wdelta[1u << BIN_MAX_LOG2_B2];
  __shared__ uint32_t s_wave[BIN_THREADS / 64];
  __shared__ __attribute__((aligned(16))) unsigned long long s_words[BIN2_WORDS]; // the tile's packed words, bucket after bucket
  __shared__ uint16_t s_wb[BIN2_WORDS];                                            // the bucket of each word
  const uint32_t tid = threadIdx.x;
  // Workgroup -> (level-1 bucket, tile): the tiles of one level-1 bucket go to workgroups L, L + 8, L + 16, ... -- one XCD, as
  // workgroups are dealt out today (speed only: any placement gives the same bits).  A level-2 bucket grows by runs of a few
  // words at arbitrary 8-byte offsets; with its writers spread over the eight L2s every run left each L2 as pieces
  // of 128-byte lines, with one L2 behind a bucket the neighbouring runs meet there and whole lines go out.
  const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3;
  const uint32_t b1 = (slot / P.tiles2) * 8u + xcd;
  if (b1 >= P.B1) return;
  const uint32_t n1 = min(P.cnt1[(uint64_t)b1 * BIN_CNT_STRIDE], P.cap1);
  const uint32_t t0 = (slot % P.tiles2) * KEY_TILE;
  if (t0 >= n1) return;
  const uint32_t tile_len = min(KEY_TILE, n1 - t0);
  const uint32_t B2 = 1u << P.log2_b2;
  if (tid < B2) s_cnt[tid] = 0;
  {
    uint4* z = reinterpret_cast<uint4*>(s_words);
    for (uint32_t i = tid; i < BIN2_WORDS / 2; i += BIN_THREADS) z[i] = make_uint4(0, 0, 0, 0);
  }
  __syncthreads();
  const uint32_t* in = P.in1 + (uint64_t)b1 * P.cap1 + t0;
  if (tile_len == KEY_TILE) // (uniform)
    bin2_tile<true>(P, in, tile_len, b1, s_cnt, s_tab, s_wdelta, s_wave, s_words, s_wb);
  else
    bin2_tile<false>(P, in, tile_len, b1, s_cnt, s_tab, s_wdelta, s_wave, s_words, s_wb);
}

// one workgroup per final bucket: residues -> LDS bitmap -> OR into the filter
// was_empty: the filter held no bit before this build; unless `dirty` says that indices were set directly meanwhile, the bucket's
// words are then stored without being read
// PACKED: the bucket holds k_bin2's packed words (cap and the count in words), else 32-bit residues (k_bin1's, one level)
// AND: the bitmap is AND-ed into the filter instead (nts_bf_insert_and; BinLate): a bucket without residues clears its slice, and
// nothing is touched when `dirty` is up.  and_sparse (the host knows that the running filter holds few bits -- BASELINE config 4
// after its first level): the slice is looked at first and a slice without a bit is left as it is, residues unread.
template <bool PACKED, bool AND>
__global__ __launch_bounds__(BIN3_THREADS) void k_bin3(const uint32_t* __restrict__ cnt, uint32_t cnt_stride, const uint32_t* __restrict__ in,
                                                       uint32_t cap, uint32_t* __restrict__ bf, uint64_t total_words, uint32_t was_empty,
                                                       const uint32_t* __restrict__ dirty, uint32_t and_sparse, unsigned long long* __restrict__ pop)
{
  extern __shared__ __attribute__((aligned(16))) uint32_t s_bits[]; // BIN_FINAL_WORDS
  // `pop`: the set bits of the slices as this kernel leaves them, summed (one atomic per workgroup): in the store-only and in the
  // AND finish the filter's popcount -- what the reference prints after every level (cpp:132,154,162) -- needs no pass of its own
  // (2.5 ms per 14.8 GB).  k_bin_late adds the bits it sets afterwards.
  __shared__ uint32_t s_pop;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) s_pop = 0;
  const uint64_t fb = blockIdx.x;
  const uint32_t n = min(cnt[fb * cnt_stride], cap);
  const uint64_t w0 = fb * (uint64_t)BIN_FINAL_WORDS;
  if (AND) {
    if (w0 >= total_words || *dirty != 0u) return; // (uniform; the buckets behind the filter's last word hold nothing)
  } else if (n == 0)
    return;
  const uint32_t n_words = (uint32_t)min((uint64_t)BIN_FINAL_WORDS, total_words - w0);
  uint4* dst = reinterpret_cast<uint4*>(bf + w0); // w0 is a multiple of 32768 words: 16-byte aligned
  uint4* z = reinterpret_cast<uint4*>(s_bits);
  if (AND && (n == 0 || and_sparse)) {
    uint32_t any = 0;
    for (uint32_t i = tid; i < n_words / 4; i += BIN3_THREADS) {
      const uint4 o = dst[i];
      const uint32_t a = o.x | o.y | o.z | o.w;
      any |= a;
      if (n == 0 && a) dst[i] = make_uint4(0, 0, 0, 0);
    }
    for (uint32_t i = (n_words & ~3u) + tid; i < n_words; i += BIN3_THREADS) {
      const uint32_t a = bf[w0 + i];
      any |= a;
      if (n == 0 && a) bf[w0 + i] = 0u;
    }
    if (n == 0) return;
    if (!__syncthreads_or((int)(any != 0u))) return;
  }
  for (uint32_t i = tid; i < BIN_FINAL_WORDS / 4; i += BIN3_THREADS) z[i] = make_uint4(0, 0, 0, 0);
  __syncthreads();
  auto set_bit = [&](uint32_t r) { atomicOr(&s_bits[r >> 5], 1u << (r & 31u)); };
  auto set_word = [&](uint32_t lo, uint32_t hi) { // residues at bits 0..18, 19..37, 38..56, their valid bits at 57..59
    constexpr uint32_t M = (1u << BIN_FINAL_SHIFT) - 1u;
    if (hi & (1u << 25)) set_bit(lo & M);
    if (hi & (1u << 26)) set_bit(((lo >> 19) | (hi << 13)) & M);
    if (hi & (1u << 27)) set_bit((hi >> 6) & M);
  };
  // sixteen bytes at a time, four such loads per lane in flight (one load, its wait, one LDS atomic per turn kept a
  // single 256-byte request per wave on its way); the index is clamped so that the loads stay unconditional and go out together
  const uint32_t* src = in + fb * (uint64_t)cap * (PACKED ? 2u : 1u);
  const uint4* src4 = reinterpret_cast<const uint4*>(src); // (cap is a multiple of four entries / two words)
  const uint32_t n4 = PACKED ? n >> 1 : n >> 2;
  for (uint32_t base = 0; base < n4; base += 4u * BIN3_THREADS) {
    uint4 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = src4[min(base + (uint32_t)q * BIN3_THREADS + tid, n4 - 1u)];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (base + (uint32_t)q * BIN3_THREADS + tid < n4) {
        if (PACKED) {
          set_word(v[q].x, v[q].y);
          set_word(v[q].z, v[q].w);
        } else {
          set_bit(v[q].x);
          set_bit(v[q].y);
          set_bit(v[q].z);
          set_bit(v[q].w);
        }
      }
  }
  if (PACKED) {
    if (tid == 0 && (n & 1u)) set_word(src[2u * (n - 1u)], src[2u * (n - 1u) + 1u]);
  } else if (tid < (n & 3u)) {
    set_bit(src[(n & ~3u) + tid]);
  }
  __syncthreads();
  uint32_t mine = 0;
  auto add_pop = [&]() { // (uniform call)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
    if ((tid & 63u) == 0u && mine) atomicAdd(&s_pop, mine);
    __syncthreads();
    if (tid == 0 && s_pop) atomicAdd(pop, (unsigned long long)s_pop);
  };
  if (AND) {
    for (uint32_t i = tid; i < n_words / 4; i += BIN3_THREADS) {
      const uint4 o = dst[i];
      if ((o.x | o.y | o.z | o.w) == 0u) continue; // (nothing to keep: no store)
      const uint4 v = z[i];
      const uint4 a = make_uint4(o.x & v.x, o.y & v.y, o.z & v.z, o.w & v.w);
      dst[i] = a;
      mine += __popc(a.x) + __popc(a.y) + __popc(a.z) + __popc(a.w);
    }
    for (uint32_t i = (n_words & ~3u) + tid; i < n_words; i += BIN3_THREADS)
      if (bf[w0 + i]) {
        const uint32_t a = bf[w0 + i] & s_bits[i];
        bf[w0 + i] = a;
        mine += __popc(a);
      }
    add_pop();
    return;
  }
  if (was_empty && *dirty == 0u) { // (uniform)
    for (uint32_t i = tid; i < n_words / 4; i += BIN3_THREADS) {
      const uint4 a = z[i];
      dst[i] = a;
      mine += __popc(a.x) + __popc(a.y) + __popc(a.z) + __popc(a.w);
    }
    for (uint32_t i = (n_words & ~3u) + tid; i < n_words; i += BIN3_THREADS) {
      bf[w0 + i] = s_bits[i];
      mine += __popc(s_bits[i]);
    }
    add_pop();
    return;
  }
  for (uint32_t i = tid; i < n_words / 4; i += BIN3_THREADS) {
    const uint4 v = z[i];
    if ((v.x | v.y | v.z | v.w) == 0u) continue;
    uint4 o = dst[i];
    o.x |= v.x;
    o.y |= v.y;
    o.z |= v.z;
    o.w |= v.w;
    dst[i] = o;
  }
  for (uint32_t i = (n_words & ~3u) + tid; i < n_words; i += BIN3_THREADS)
    if (s_bits[i]) bf[w0 + i] |= s_bits[i];
}

// the indices parked by bin_set_late, once k_bin3 is through
__global__ __launch_bounds__(256) void k_bin_late(const uint64_t* __restrict__ list, const unsigned long long* __restrict__ count, uint64_t cap,
                                                  uint32_t* __restrict__ bf, unsigned long long* __restrict__ pop)
{
  const uint64_t n = min((uint64_t)*count, cap);
  uint32_t fresh = 0; // bits this lane turned on (the returning atomic tells; duplicates of an index lose)
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const uint64_t idx = list[i];
    uint32_t* w = &bf[idx >> 5];
    const uint32_t bit = 1u << (idx & 31);
    if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) && !(atomicOr(w, bit) & bit)) ++fresh;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) fresh += __shfl_down(fresh, off, 64);
  if ((threadIdx.x & 63u) == 0u && fresh) atomicAdd(pop, (unsigned long long)fresh);
}

constexpr uint64_t BIN_LATE_MIN = 1ull << 20; // entries of the list of bucket-bypassing indices: this, or one per 24 k-mers (1 GB at 3 Gbp)

// The geometry of a build: what bf_insert_binned launches with, from the numbers alone (exported as nts_bf_bin_plan for the CPU suite).
struct BinPlan
{
  uint64_t F;        // final buckets that hold filter bits: ceil(bits / 2^BIN_FINAL_SHIFT)
  uint32_t log2_b2;  // level-2 buckets per level-1 bucket (0: one partition level)
  uint32_t B2, B1;   // B1 = ceil(F / B2) <= BIN_MAX_B1
  uint64_t n_final;  // B1 * B2 >= F final buckets are launched; those from F on lie behind the filter's end and stay empty
  uint64_t cap1;     // residues per level-1 bucket (a multiple of four)
  uint64_t cap2;     // packed words per level-2 bucket (even; 0 with one level)
  uint64_t tiles;    // k_bin1's tiles of KEY_TILE k-mers
  uint64_t tiles2;   // k_bin2's tiles per level-1 bucket
  uint32_t idx32;    // B1 * cap1 < 2^32: a residue's place in out1 is a 32-bit index
};

// returns 0 when the binned build applies to V valid k-mers and a filter of `bytes` bytes, 1 when it does not (V = 0 included: nothing to build)
int bf_bin_plan(uint64_t V, uint64_t bytes, uint32_t k, bool forced, bool and_mode, BinPlan& p)
{
  p = BinPlan{};
  if (V == 0 || bytes == 0 || bytes > (1ull << 60)) return 1;
  const uint64_t bits = bytes * 8;
  const uint64_t F = (bits + (1ull << BIN_FINAL_SHIFT) - 1) >> BIN_FINAL_SHIFT; // final buckets
  if (V >= 0xFF000000ULL) return 1;                    // 32-bit bucket cursors
  if (!forced && (V < (1u << 22) || F < 64)) return 1; // too small to pay for three passes
  uint32_t log2_b2 = 0;
  // (the ceiling, as B1 below: F >> log2_b2 let F = 512 * 2^j + r, 0 < r < 2^j, through with 513 buckets for k_bin1's tables of 512)
  while (log2_b2 <= BIN_MAX_LOG2_B2 && ((F + (1ull << log2_b2) - 1) >> log2_b2) > BIN_MAX_B1) ++log2_b2;
  if (log2_b2 > BIN_MAX_LOG2_B2) return 1;             // filter beyond 2^37 bits (17 GB)
  if (and_mode && k > FAST_K_MAX) return 1;            // (k_bin1_long sets every index directly)
  const uint32_t B2 = 1u << log2_b2;
  const uint32_t B1 = (uint32_t)((F + B2 - 1) >> log2_b2);
  if (B1 > BIN_MAX_B1) return 1;                       // (k_bin1's s_cnt and s_gbase)
  const uint64_t n_final = (uint64_t)B1 << log2_b2;
  // capacities: mean + slack (uniform hashes: sigma ~ sqrt(mean)); what does not fit is OR-ed directly
  const uint64_t mean1 = V / B1 + 1, mean2 = V / F + 1;
  const uint64_t cap1 = (mean1 + mean1 / 8 + 4096 + 3) & ~3ull;
  // level-2 buckets hold packed words (three residues each); every tile of the level-1 bucket may leave a partly filled word
  const uint64_t mean2w = mean2 / 3 + (mean1 / KEY_TILE + 2);
  const uint64_t cap2 = log2_b2 ? ((mean2w + mean2w / 4 + 512 + 1) & ~1ull) : 0;
  if (cap1 >= 0x7FFFFFFFULL || cap2 >= 0x7FFFFFFFULL) return 1;
  if (((uint64_t)cap2 << log2_b2) >= (1ull << 30)) return 1; // (k_bin2 addresses the level-2 buckets of a level-1 bucket with 32-bit offsets)
  const uint64_t tiles = (V + KEY_TILE - 1) / KEY_TILE;
  const uint64_t tiles2 = (cap1 + KEY_TILE - 1) / KEY_TILE;
  if (tiles > 0x7FFFFFFFULL || tiles2 * (B1 + 8ull) > 0x7FFFFFFFULL || B1 > 65535 || n_final > 0x7FFFFFFFULL) return 1;
  p.F = F;
  p.log2_b2 = log2_b2;
  p.B2 = B2;
  p.B1 = B1;
  p.n_final = n_final;
  p.cap1 = cap1;
  p.cap2 = cap2;
  p.tiles = tiles;
  p.tiles2 = tiles2;
  p.idx32 = ((uint64_t)B1 * cap1 < (1ull << 32)) ? 1u : 0u;
  return 0;
}

// returns NTS_OK when the binned build ran, 1 when it does not apply (caller uses the atomic kernel)
// was_empty: no bit of the filter is set (a new or cleared filter: every build of the pipeline)
// and_mode: 0 = OR into the filter, 1 = AND into it (BinLate), 2 = the same with the host's word that the filter holds few bits.
// late_ctl (pinned host, 8 words; may be NULL): receives {dirty, -, count lo, count hi, popcount lo, popcount hi} behind the build (the
// caller synchronises); word 6 is set at once: 1 = the popcount words will hold the filter's popcount (store-only / AND finish)
int bf_insert_binned(nts_ctx* ctx, nts_bf* bf, const nts_genome* g, const GenomeTables& T, uint32_t k, bool forced, bool was_empty, int and_mode = 0,
                     uint32_t* late_ctl = nullptr)
{
  const RunTable& rt = T.rt;
  const uint64_t V = rt.n_valid;
  if (V == 0) return NTS_OK;
  BinPlan plan;
  ctx->last_bin1_grid = 0;
  if (bf_bin_plan(V, bf->bytes, k, forced, and_mode != 0, plan)) return 1;
  ctx->last_bin_b1 = plan.B1;
  ctx->last_bin_log2_b2 = plan.log2_b2;
  const uint64_t bits = bf->bytes * 8;
  const uint32_t log2_b2 = plan.log2_b2, B1 = plan.B1;
  const uint64_t n_final = plan.n_final, cap1 = plan.cap1, cap2 = plan.cap2, tiles = plan.tiles, tiles2 = plan.tiles2;
  NTS_WS(d_cnt1, uint32_t*, "bin_cnt1", (uint64_t)B1 * BIN_CNT_STRIDE * 4);
  NTS_WS(d_out1, uint32_t*, "bin_out1", (uint64_t)B1 * cap1 * 4);
  uint32_t* d_cnt2 = nullptr;
  uint32_t* d_out2 = nullptr;
  if (log2_b2) {
    d_cnt2 = (uint32_t*)ws_get(ctx, "bin_cnt2", n_final * 4);
    d_out2 = (uint32_t*)ws_get(ctx, "bin_out2", n_final * cap2 * 8);
    if (!d_cnt2 || !d_out2) return NTS_ENOMEM;
  }
  const size_t lds3 = (size_t)BIN_FINAL_WORDS * 4;
  if (!ctx->bin_lds_set) {
    HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_bin3<true, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds3));
    HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_bin3<false, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds3));
    HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_bin3<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds3));
    HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_bin3<false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds3));
    ctx->bin_lds_set = true;
  }
  // store-only finish (see BinLate); NTS_BIN_STORE=0: always read and OR (tests)
  const bool store_only = !and_mode && was_empty && k <= FAST_K_MAX && !(NTS_KNOB("NTS_BIN_STORE") && atoi(NTS_KNOB("NTS_BIN_STORE")) == 0);
  uint32_t* d_dirty = (uint32_t*)ws_get(ctx, "bin_late_ctl", 32);
  if (!d_dirty) return NTS_ENOMEM;
  HIP_TRY(ctx, hipMemsetAsync(d_dirty, 0, 32, ctx->stream));
  unsigned long long* d_pop = (unsigned long long*)(d_dirty + 4);
  BinLate late = { nullptr, (unsigned long long*)(d_dirty + 2), 0, d_dirty, and_mode ? 1u : 0u };
  if (store_only || and_mode) {
    const uint64_t late_cap = std::max<uint64_t>(BIN_LATE_MIN, V / 24);
    late.list = (uint64_t*)ws_get(ctx, "bin_late", late_cap * 8);
    if (!late.list) return NTS_ENOMEM;
    late.cap = NTS_KNOB("NTS_BIN_LATE_CAP") ? std::min<uint64_t>(late_cap, strtoull(NTS_KNOB("NTS_BIN_LATE_CAP"), nullptr, 10)) : late_cap; // (tests: a list that runs full)
  }
  HIP_TRY(ctx, hipMemsetAsync(d_cnt1, 0, (uint64_t)B1 * BIN_CNT_STRIDE * 4, ctx->stream));
  if (log2_b2) HIP_TRY(ctx, hipMemsetAsync(d_cnt2, 0, n_final * 4, ctx->stream));
  if (int rc_pk = ensure_pack(ctx, g)) return rc_pk;
  BinParams P;
  P.code = g->d_code + PAD;
  P.pack = g->d_pack;
  P.run_pos = T.d_run_pos;
  P.run_vstart = T.d_run_vstart;
  P.n_runs = T.n_runs;
  P.n_valid = V;
  if (int rc_hp = hash_params_for(ctx, k, &P.hp)) return rc_hp;
  P.fm = make_fastmod(bits);
  P.bf = bf->d_words;
  P.sh1 = BIN_FINAL_SHIFT + log2_b2;
  P.B1 = B1;
  P.cnt1 = d_cnt1;
  P.out1 = d_out1;
  P.cap1 = (uint32_t)cap1;
  // NTS_BIN_IDX32=0: the 64-bit place whatever the plan says (tests: the path of B1 * cap1 >= 2^32 on a small genome; it is the
  // general one -- s_gbase without b * cap1, every store through (uint64_t)b * cap1 + pos and its capacity test)
  P.idx32 = (NTS_KNOB("NTS_BIN_IDX32") && atoi(NTS_KNOB("NTS_BIN_IDX32")) == 0) ? 0u : plan.idx32;
  ctx->last_bin_idx32 = P.idx32;
  P.late = late;
  ScopedTimer t(ctx, and_mode ? "bf_insert_and" : "bf_insert", true);
  if (k > FAST_K_MAX) {
    NTS_LAUNCH(k_bin1_long, dim3((uint32_t)tiles), dim3(BIN1_THREADS), 0, ctx->stream, P);
  } else {
    if (ctx->n_cus == 0) {
      hipDeviceProp_t prop;
      HIP_TRY(ctx, hipGetDeviceProperties(&prop, ctx->device));
      ctx->n_cus = (uint32_t)prop.multiProcessorCount;
    }
    const uint32_t per_cu = NTS_KNOB("NTS_BIN1_PER_CU") ? (uint32_t)std::max(1, atoi(NTS_KNOB("NTS_BIN1_PER_CU"))) : 2u; // (workgroups that fit a CU)
    uint32_t n_wg1 = (uint32_t)std::min<uint64_t>(tiles, (uint64_t)ctx->n_cus * per_cu);
    if (NTS_KNOB("NTS_BIN1_GRID")) n_wg1 = (uint32_t)std::min<uint64_t>(tiles, (uint64_t)std::max(1, atoi(NTS_KNOB("NTS_BIN1_GRID")))); // (tests: several turns per workgroup on a small genome)
    const dim3 grid1(n_wg1);
    ctx->last_bin1_grid = n_wg1;
    if (P.fm.form == 2)
      NTS_LAUNCH(k_bin1<2>, grid1, dim3(BIN1_THREADS), 0, ctx->stream, P);
    else if (P.fm.form == 1)
      NTS_LAUNCH(k_bin1<1>, grid1, dim3(BIN1_THREADS), 0, ctx->stream, P);
    else
      NTS_LAUNCH(k_bin1<0>, grid1, dim3(BIN1_THREADS), 0, ctx->stream, P);
  }
  const uint32_t* cnt_final = d_cnt1;
  const uint32_t* in_final = d_out1;
  uint32_t cap_final = (uint32_t)cap1;
  if (log2_b2) {
    Bin2Params Q;
    Q.cnt1 = d_cnt1;
    Q.in1 = d_out1;
    Q.cap1 = (uint32_t)cap1;
    Q.log2_b2 = log2_b2;
    Q.cnt2 = d_cnt2;
    Q.out2 = d_out2;
    Q.cap2 = (uint32_t)cap2;
    Q.bf = bf->d_words;
    Q.late = late;
    Q.B1 = B1;
    Q.tiles2 = (uint32_t)tiles2;
    NTS_LAUNCH(k_bin2, dim3((uint32_t)(tiles2 * ((B1 + 7u) & ~7u))), dim3(BIN_THREADS), 0, ctx->stream, Q);
    cnt_final = d_cnt2;
    in_final = d_out2;
    cap_final = (uint32_t)cap2;
  }
  const uint64_t total_words = (bf->bytes + 3) / 4; // any byte count: the allocation is padded to 16 bytes, the pad stays zero
  const uint32_t sparse = and_mode == 2 ? 1u : 0u;
#define BIN3_LAUNCH(PACKED, AND, stride)                                                                                                     \
  NTS_LAUNCH((k_bin3<PACKED, AND>), dim3((uint32_t)n_final), dim3(BIN3_THREADS), lds3, ctx->stream, cnt_final, stride, in_final, cap_final, \
                     bf->d_words, total_words, store_only ? 1u : 0u, d_dirty, sparse, d_pop)
  if (log2_b2) {
    if (and_mode)
      BIN3_LAUNCH(true, true, 1u);
    else
      BIN3_LAUNCH(true, false, 1u);
  } else {
    if (and_mode)
      BIN3_LAUNCH(false, true, BIN_CNT_STRIDE);
    else
      BIN3_LAUNCH(false, false, BIN_CNT_STRIDE);
  }
#undef BIN3_LAUNCH
  if (store_only || and_mode) NTS_LAUNCH(k_bin_late, dim3(2048), dim3(256), 0, ctx->stream, late.list, late.count, late.cap, bf->d_words, d_pop);
  if (late_ctl) {
    HIP_TRY(ctx, hipMemcpyAsync(late_ctl, d_dirty, 24, hipMemcpyDeviceToHost, ctx->stream)); // (words 0-5; word 6 is the host's)
    late_ctl[6] = (store_only || and_mode) ? 1u : 0u; // (words 4-5 will hold the filter's popcount unless `dirty` came up)
  }
  HIP_TRY(ctx, hipGetLastError());
  return NTS_OK;
}

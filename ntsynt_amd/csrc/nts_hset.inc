// ---- an exact set of 64-bit hashes on the device, and the sweep of intervals against it (nts_hset_*; ntsynt_amd/gaps.py block_links) ----
// docs/design/04_11_gap_block_links.md.  The gaps' sampled hashes are a few per cent of a genome's; the k-mers of the BLOCKS that carry
// one of them are found by sweeping the block intervals against the set of those hashes instead of the common filter: the records then
// scale with the gaps, and the probes go to a table of 16 bytes per member, which the L2 and the Infinity Cache hold, instead of a filter
// of gigabytes.
//   the table: open addressing with linear probing, one uint64 per slot, 2^m slots with 2^m >= 2 n (at most half full; at least 64).  A
//     slot holds the member itself; HSET_EMPTY = 2^64 - 1 marks a free one, and whether 2^64 - 1 is a MEMBER is one flag beside the
//     table (has_max), set on the host from the input.  The home slot is the top m bits of h * 0x9E3779B97F4A7C15: every bit of h
//     reaches them, so hashes under a sampling threshold (top bits zero) and hashes that differ in a few bits only spread alike.
//   k_hset_insert: one lane per input value; 64-bit compare-and-swap (a vector atomic on global memory) of HSET_EMPTY against the value
//     from the home slot on; a slot that already holds the value ends the walk (duplicates).  At most half full: a walk ends.  Slot
//     order depends on which lane comes first; membership does not.
//   k_hset_contains: one lane per query, the walk of hset_walk.
//   k_hset_sample<WRITE>: nts_bf_sample.inc's frame (sample_tile: count launch, write launch, no atomic) with HsetProbe: the load of a
//     k-mer's home slot is issued as it is rolled, behind `h0 <= thresh`; after the batch's eighth k-mer the loads are looked at: equal
//     -> member, empty -> not, another member -> the walk goes on from the next slot (at load 1/2 a miss meets an occupied home slot
//     half of the time and an occupied second slot far less often).
// Experiments build only: NTS_HSET_SAMPLE_SLICE = tiles per launch (default 2^23), as NTS_BF_SAMPLE_SLICE.

constexpr uint64_t HSET_EMPTY = ~0ULL;
constexpr uint64_t HSET_MULT = 0x9E3779B97F4A7C15ULL;
constexpr uint32_t HSET_MIN_LOG2 = 6;
constexpr uint64_t HSET_MAX_N = (uint64_t)1 << 31; // 2^32 slots of 8 bytes

struct HsetView // what a kernel takes
{
  const uint64_t* __restrict__ slots;
  uint64_t mask; // n_slots - 1
  uint32_t shift;
  uint32_t has_max;
  __device__ __forceinline__ uint64_t home(uint64_t h) const { return (h * HSET_MULT) >> shift; }
};

constexpr uint64_t HSET_NONE = ~0ULL; // hset_find's "not a member" (no table has 2^64 slots)

// the one walk, from slot s, which was found to hold v, for h (!= HSET_EMPTY); what it answers is the caller's: As::hit(slot) / As::miss()
template <typename As>
__device__ __forceinline__ auto hset_walk_as(const HsetView& t, uint64_t h, uint64_t s, uint64_t v) -> decltype(As::miss())
{
  for (;;) {
    if (v == h) return As::hit(s);
    if (v == HSET_EMPTY) return As::miss();
    s = (s + 1) & t.mask;
    v = t.slots[s];
  }
}
struct HsetAsHeld
{
  static __device__ __forceinline__ bool hit(uint64_t) { return true; }
  static __device__ __forceinline__ bool miss() { return false; }
};
struct HsetAsSlot
{
  static __device__ __forceinline__ uint64_t hit(uint64_t s) { return s; }
  static __device__ __forceinline__ uint64_t miss() { return HSET_NONE; }
};

// is h (!= HSET_EMPTY) in the table, given that slot s was found to hold v
__device__ __forceinline__ bool hset_walk(const HsetView& t, uint64_t h, uint64_t s, uint64_t v) { return hset_walk_as<HsetAsHeld>(t, h, s, v); }

// the slot that holds it, HSET_NONE when the table does not have it (nts_hcount.inc: a member's count lies at its slot's index)
__device__ __forceinline__ uint64_t hset_find(const HsetView& t, uint64_t h, uint64_t s, uint64_t v) { return hset_walk_as<HsetAsSlot>(t, h, s, v); }

__global__ __launch_bounds__(256) void k_hset_insert(const uint64_t* __restrict__ in, uint64_t n, uint64_t* slots, uint64_t mask, uint32_t shift)
{
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t h = in[i];
  if (h == HSET_EMPTY) return; // (the flag beside the table answers for it)
  uint64_t s = (h * HSET_MULT) >> shift;
  for (;;) {
    const uint64_t was = atomicCAS((unsigned long long*)(slots + s), (unsigned long long)HSET_EMPTY, (unsigned long long)h);
    if (was == HSET_EMPTY || was == h) return;
    s = (s + 1) & mask;
  }
}

__global__ __launch_bounds__(256) void k_hset_contains(HsetView t, const uint64_t* __restrict__ q, uint64_t n, uint8_t* __restrict__ out)
{
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t h = q[i];
  bool in = t.has_max != 0;
  if (h != HSET_EMPTY) {
    const uint64_t s = t.home(h);
    in = hset_walk(t, h, s, t.slots[s]);
  }
  out[i] = in ? 1 : 0;
}

struct HsetProbe // membership in the table; HSET_EMPTY itself is answered by the flag
{
  HsetView t;
  uint64_t key[BFS_BATCH], got[BFS_BATCH];
  __device__ __forceinline__ void issue(int u, uint64_t h0)
  {
    key[u] = h0;
    got[u] = t.slots[t.home(h0)];
  }
  __device__ __forceinline__ void skip(int u)
  {
    key[u] = 0; // (0 against an empty slot: not held, no walk)
    got[u] = HSET_EMPTY;
  }
  __device__ __forceinline__ bool held(int u) const
  {
    const uint64_t h = key[u];
    if (h == HSET_EMPTY) return t.has_max != 0; // (the one key the table cannot hold)
    if (got[u] == h) return true;
    if (got[u] == HSET_EMPTY) return false;
    const uint64_t s = (t.home(h) + 1) & t.mask;
    return hset_walk(t, h, s, t.slots[s]);
  }
};

template <bool WRITE>
__global__ __launch_bounds__(HASH_THREADS) void k_hset_sample(const uint8_t* __restrict__ code, const IvTile* __restrict__ tiles,
                                                              const uint32_t* __restrict__ tile_off0, HsetView set, uint64_t thresh,
                                                              uint32_t* __restrict__ tile_cnt, const uint64_t* __restrict__ tile_at,
                                                              SampleRec* __restrict__ out, uint64_t n_out, HashParams hp)
{
  HsetProbe probe{ set };
  sample_tile<WRITE>(code, tiles, tile_off0, probe, thresh, tile_cnt, tile_at, out, n_out, hp);
}

inline HsetView hset_view(const nts_hset* s)
{
  return HsetView{ s->d_slots, s->n_slots - 1, s->shift, s->has_max ? 1u : 0u };
}

int hset_build_run(nts_ctx* ctx, const uint64_t* h, uint64_t n, nts_hset** out)
{
  *out = nullptr;
  if (n > HSET_MAX_N) return fail(ctx, NTS_ERANGE, "nts_hset_build: more than 2^31 values (the table would pass 2^32 slots)");
  uint32_t log2 = HSET_MIN_LOG2;
  while (((uint64_t)1 << log2) < 2 * n) ++log2;
  nts_hset* s = new nts_hset();
  s->n_slots = (uint64_t)1 << log2;
  s->shift = 64 - log2;
  s->n_in = n;
  s->device = ctx->device;
  for (uint64_t i = 0; i < n && !s->has_max; ++i) s->has_max = h[i] == HSET_EMPTY;
  hipError_t e = dev_malloc((void**)&s->d_slots, s->n_slots * 8);
  if (e != hipSuccess) {
    delete s;
    HIP_TRY(ctx, e);
  }
  uint64_t* d_in = nullptr;
  if (n) {
    d_in = (uint64_t*)ws_get(ctx, "hset_in", n * 8);
    if (!d_in) {
      dev_free(s->d_slots);
      delete s;
      return NTS_ENOMEM;
    }
  }
  if (n) e = hipMemcpyAsync(d_in, h, n * 8, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    ScopedTimer t(ctx, "hset_build", true); // (the table: clearing it and the inserts, not the upload of the values)
    e = hipMemsetAsync(s->d_slots, 0xFF, s->n_slots * 8, ctx->stream);
    if (e == hipSuccess && n) {
      NTS_LAUNCH(k_hset_insert, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const uint64_t*)d_in, n, s->d_slots, s->n_slots - 1, s->shift);
      e = hipGetLastError();
    }
  }
  const hipError_t e_sync = hipStreamSynchronize(ctx->stream); // (the copy reads the caller's array)
  if (e != hipSuccess || e_sync != hipSuccess) {
    dev_free(s->d_slots);
    delete s;
  }
  HIP_TRY(ctx, e);
  HIP_TRY(ctx, e_sync);
  *out = s;
  return NTS_OK;
}

int hset_contains_run(nts_ctx* ctx, const nts_hset* s, const uint64_t* h, uint64_t n, uint8_t* out)
{
  if (n == 0) return NTS_OK;
  if (n > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_hset_contains: 2^32 queries or more in one call");
  NTS_WS(d_q, uint64_t*, "hset_q", n * 8);
  NTS_WS(d_a, uint8_t*, "hset_a", n);
  hipError_t e = hipMemcpyAsync(d_q, h, n * 8, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    ScopedTimer t(ctx, "hset_contains");
    NTS_LAUNCH(k_hset_contains, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, hset_view(s), (const uint64_t*)d_q, n, d_a);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_a, n, hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t e_sync = hipStreamSynchronize(ctx->stream);
  HIP_TRY(ctx, e);
  HIP_TRY(ctx, e_sync);
  return NTS_OK;
}

int hset_sample_intervals_run(nts_ctx* ctx, const nts_genome* g, uint32_t k, const nts_hset* s, uint64_t rate, const nts_interval* iv, uint64_t n_iv,
                              uint64_t* n_sampled, nts_sample** out, uint64_t* n_out)
{
  const HsetView set = hset_view(s);
  const uint8_t* code = g->d_code + PAD;
  const SampleNames nm{ "nts_hset_sample_intervals", "hset_sample_count", "hset_sample_write", NTS_KNOB("NTS_HSET_SAMPLE_SLICE") };
  return sample_intervals_run(ctx, g, k, rate, iv, n_iv, n_sampled, out, n_out, nm,
                              [&](bool write, uint32_t n, const IvTile* d_tiles, const uint32_t* d_off0, uint64_t thresh, uint32_t* d_cnt,
                                  const uint64_t* d_at, SampleRec* d_out, uint64_t total, const HashParams& hp) {
                                if (write)
                                  NTS_LAUNCH(k_hset_sample<true>, dim3(n), dim3(HASH_THREADS), 0, ctx->stream, code, d_tiles, d_off0, set, thresh, d_cnt, d_at,
                                             d_out, total, hp);
                                else
                                  NTS_LAUNCH(k_hset_sample<false>, dim3(n), dim3(HASH_THREADS), 0, ctx->stream, code, d_tiles, d_off0, set, thresh, d_cnt, d_at,
                                             d_out, total, hp);
                              });
}

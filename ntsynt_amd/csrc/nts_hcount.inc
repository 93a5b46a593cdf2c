// ---- how often the members of a hash set occur: a counting table beside the set, and the sweep that adds to it (nts_hcount_*; ----
// ntsynt_amd/gaps.py copies).  docs/design/04_12_gap_copies.md.  The link reports ask "is this k-mer of a gap there"; whether a gap is
// a repeat asks "how many times", genome-wide.  The set (nts_hset.inc) stays what it is; the counts lie beside it:
//   the table: one uint32 per slot of the set's table, and one more, at index n_slots, for the key 2^64 - 1, which the table cannot
//     hold (has_max).  A member's count is found by the set's own walk (hset_find: hset_walk that says where), so counts are only
//     ever addressed by key -- the slot order of the set differs from run to run, a key's count does not.
//   k_hcount_add / k_hcount_read: one lane per value of a host array, hset_slot_of, then one atomicAdd of 1 / one load.
//   k_hset_count: the tile sweep (nts_tile_sweep.inc) with HsetProbe's loads -- the home slot's load is issued as the k-mer is rolled,
//     behind `h0 <= thresh`; after the batch's eighth k-mer the eight are resolved to slots (HcountProbe::slot) -- and per hit ONE
//     atomicAdd of 1 on the uint32 at that slot: a vector atomic on global memory whose result is not used (no return value is asked
//     for, the lane does not wait for it).  The tile's hits go the way of the sampling sweep's count launch: lanes -> wave ->
//     workgroup, one plain store per tile (block_sum_store), added up per interval on the host (iv_counts_back).  Integer adds
//     commute: the counts are exact and the same from run to run, whatever order the waves come in.
//   contention: every occurrence of one k-mer adds to one address.  The adds are NOT merged within a lane's batch or within the wave:
//     the plain version comes first, and merging is for the day a measurement on a genome with satellite arrays asks for it (the
//     design note says what is and is not measured).  The atomic returns nothing, so no lane waits on a contended address.
//   range: counts are 32-bit.  The counter keeps on the host how many values and k-mers it has been offered since the last clear
//     (every k-mer of a sweep, hit or not: known before the launch); a call that would bring the total to 2^32 is refused.
//   k_hset_sample_capped<WRITE>: the sampling sweep (nts_bf_sample.inc's sample_tile, as k_hset_sample) that keeps a k-mer when the set
//     has it AND its count lies in 1..cap (HcapProbe: HcountProbe's slot, then one dependent 4-byte load of the count there).  The
//     counter is only read: no atomic, the records are deterministic.  docs/design/04_13_gap_copy_sites.md.
// Experiments build only: NTS_HSET_COUNT_SLICE = tiles per launch (default 2^23), as NTS_HSET_SAMPLE_SLICE (which also cuts the capped
// sweep's launches).

// the index of h's count: its slot, n_slots for 2^64 - 1 when that is a member, HSET_NONE for a non-member
__device__ __forceinline__ uint64_t hset_slot_of(const HsetView& t, uint64_t h)
{
  if (h == HSET_EMPTY) return t.has_max ? t.mask + 1 : HSET_NONE;
  const uint64_t s = t.home(h);
  return hset_find(t, h, s, t.slots[s]);
}

__global__ __launch_bounds__(256) void k_hcount_add(HsetView t, const uint64_t* __restrict__ q, uint64_t n, uint32_t* __restrict__ cnt)
{
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t at = hset_slot_of(t, q[i]);
  if (at != HSET_NONE) atomicAdd(cnt + at, 1u);
}

__global__ __launch_bounds__(256) void k_hcount_read(HsetView t, const uint64_t* __restrict__ q, uint64_t n, const uint32_t* __restrict__ cnt,
                                                     uint32_t* __restrict__ out)
{
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t at = hset_slot_of(t, q[i]);
  out[i] = at != HSET_NONE ? cnt[at] : 0u;
}

struct HcountProbe // HsetProbe's loads, resolved to where the key's count lies instead of whether it is held
{
  HsetProbe p;
  __device__ __forceinline__ void issue(int u, uint64_t h0) { p.issue(u, h0); }
  __device__ __forceinline__ void skip(int u) { p.skip(u); }
  __device__ __forceinline__ uint64_t slot(int u) const
  {
    const uint64_t h = p.key[u];
    if (h == HSET_EMPTY) return p.t.has_max ? p.t.mask + 1 : HSET_NONE;
    if (p.got[u] == HSET_EMPTY) return HSET_NONE; // (most k-mers: over the threshold, or a miss that met a free home slot)
    return hset_find(p.t, h, p.t.home(h), p.got[u]);
  }
};

__global__ __launch_bounds__(HASH_THREADS) void k_hset_count(const uint8_t* __restrict__ code, const IvTile* __restrict__ tiles, HsetView set,
                                                             uint64_t thresh, uint32_t* __restrict__ cnt, uint32_t* __restrict__ tile_hits,
                                                             HashParams hp)
{
  __shared__ uint64_t s_tab[36];
  __shared__ uint32_t s_seq[SEQ_LDS_DWORDS];
  __shared__ uint32_t s_w[HASH_THREADS / 64];
  const IvTile tile = tiles[blockIdx.x];
  const TileLane lane = tile_enter(s_tab, s_seq, code, tile.pos, tile.len, hp);
  HcountProbe probe{ HsetProbe{ set } };
  uint32_t hits = 0;
  lane.sweep(
    hp, s_tab,
    [&](uint32_t j, int u, uint64_t h0) { // (nothing is probed for a k-mer past the lane's last)
      if (j < lane.n_mine && h0 <= thresh)
        probe.issue(u, h0);
      else
        probe.skip(u);
    },
    [&](uint32_t) {
#pragma unroll
      for (int u = 0; u < BFS_BATCH; ++u) {
        const uint64_t at = probe.slot(u);
        if (at != HSET_NONE) {
          atomicAdd(cnt + at, 1u);
          ++hits;
        }
      }
    });
  block_sum_store(hits, s_w, tile_hits + blockIdx.x);
}

constexpr uint64_t HCOUNT_LIMIT = (uint64_t)1 << 32; // what a counter may be offered between two clears

// the counter is the set's own, both live on the context's device; a call that offers `more` stays under the limit
int hcount_check(nts_ctx* ctx, const nts_hset* s, const nts_hcount* c, uint64_t more, const char* who)
{
  if (c->set != s || c->n_slots != s->n_slots) return fail(ctx, NTS_EINVAL, std::string(who) + ": the counter belongs to another set");
  if (more >= HCOUNT_LIMIT || c->offered + more >= HCOUNT_LIMIT)
    return fail(ctx, NTS_ERANGE, std::string(who) + ": 2^32 values and k-mers or more since the last clear (counts are 32-bit)");
  return NTS_OK;
}

int hcount_clear_run(nts_ctx* ctx, nts_hcount* c)
{
  hipError_t e;
  {
    ScopedTimer t(ctx, "hcount_clear", true);
    e = hipMemsetAsync(c->d_cnt, 0, (c->n_slots + 1) * 4, ctx->stream);
  }
  const hipError_t e_sync = hipStreamSynchronize(ctx->stream);
  HIP_TRY(ctx, e);
  HIP_TRY(ctx, e_sync);
  c->offered = 0;
  return NTS_OK;
}

int hcount_create_run(nts_ctx* ctx, const nts_hset* s, nts_hcount** out)
{
  *out = nullptr;
  nts_hcount* c = new nts_hcount();
  c->set = s;
  c->n_slots = s->n_slots;
  c->device = ctx->device;
  hipError_t e = dev_malloc((void**)&c->d_cnt, (c->n_slots + 1) * 4);
  if (e != hipSuccess) {
    delete c;
    HIP_TRY(ctx, e);
  }
  const int rc = hcount_clear_run(ctx, c);
  if (rc) {
    dev_free(c->d_cnt);
    delete c;
    return rc;
  }
  *out = c;
  return NTS_OK;
}

int hcount_add_run(nts_ctx* ctx, const nts_hset* s, nts_hcount* c, const uint64_t* h, uint64_t n)
{
  {
    const int rc = hcount_check(ctx, s, c, n, "nts_hcount_add"); // (before h is looked at)
    if (rc) return rc;
  }
  if (n == 0) return NTS_OK;
  NTS_WS(d_q, uint64_t*, "hset_q", n * 8);
  hipError_t e = hipMemcpyAsync(d_q, h, n * 8, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    ScopedTimer t(ctx, "hcount_add", true);
    NTS_LAUNCH(k_hcount_add, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, hset_view(s), (const uint64_t*)d_q, n, c->d_cnt);
    e = hipGetLastError();
  }
  const hipError_t e_sync = hipStreamSynchronize(ctx->stream); // (the copy reads the caller's array)
  HIP_TRY(ctx, e);
  HIP_TRY(ctx, e_sync);
  c->offered += n;
  return NTS_OK;
}

int hcount_read_run(nts_ctx* ctx, const nts_hset* s, const nts_hcount* c, const uint64_t* h, uint64_t n, uint32_t* out)
{
  {
    const int rc = hcount_check(ctx, s, c, 0, "nts_hcount_read");
    if (rc) return rc;
  }
  if (n == 0) return NTS_OK;
  if (n > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_hcount_read: 2^32 queries or more in one call");
  NTS_WS(d_q, uint64_t*, "hset_q", n * 8);
  NTS_WS(d_a, uint32_t*, "hcount_a", n * 4);
  hipError_t e = hipMemcpyAsync(d_q, h, n * 8, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    ScopedTimer t(ctx, "hcount_read", true);
    NTS_LAUNCH(k_hcount_read, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, hset_view(s), (const uint64_t*)d_q, n,
               (const uint32_t*)c->d_cnt, d_a);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_a, n * 4, hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t e_sync = hipStreamSynchronize(ctx->stream);
  HIP_TRY(ctx, e);
  HIP_TRY(ctx, e_sync);
  return NTS_OK;
}

// the host side is bf_count_intervals_run's: the cutter, one launch per slice, the tiles' hits added up per interval
int hset_count_intervals_run(nts_ctx* ctx, const nts_genome* g, uint32_t k, const nts_hset* s, nts_hcount* c, uint64_t rate, const nts_interval* iv,
                             uint64_t n_iv, uint64_t* n_hits)
{
  const char* who = "nts_hset_count_intervals";
  {
    const int rc = hcount_check(ctx, s, c, 0, who);
    if (rc) return rc;
  }
  if (n_iv == 0) return NTS_OK;
  std::vector<uint64_t> nk;
  std::vector<IvTile> tiles;
  HashParams hp;
  {
    const int rc = iv_cut_tiles(ctx, g, k, iv, n_iv, who, nk, tiles, &hp);
    if (rc) return rc;
  }
  uint64_t offered = 0;
  for (uint64_t i = 0; i < n_iv; ++i) {
    n_hits[i] = 0;
    offered += nk[i]; // (a genome's k-mers, at most once per interval: no overflow of 64 bits short of 2^32 intervals of 2^32 bases)
  }
  {
    const int rc = hcount_check(ctx, s, c, offered, who); // (before anything is launched)
    if (rc) return rc;
  }
  if (tiles.empty()) return NTS_OK;
  const HsetView set = hset_view(s);
  const uint64_t thresh = ~0ULL / rate;
  NTS_WS(d_hits, uint32_t*, "hcount_hits", tiles.size() * 4); // (before the upload: nothing may fail between the asynchronous copy out of `tiles` and the synchronise of iv_counts_back)
  IvTile* d_tiles = nullptr;
  {
    const int rc = ws_upload(ctx, "hcount_tiles", tiles, &d_tiles);
    if (rc) return rc;
  }
  c->offered += offered; // (from here on adds may have landed, whatever the launches report)
  iv_for_slices(ctx, "hcount_sweep", tiles.size(), iv_slice(NTS_KNOB("NTS_HSET_COUNT_SLICE")), [&](uint64_t t0, uint32_t nt) {
    NTS_LAUNCH(k_hset_count, dim3(nt), dim3(HASH_THREADS), 0, ctx->stream, g->d_code + PAD, d_tiles + t0, set, thresh, c->d_cnt, d_hits + t0, hp);
  });
  std::vector<uint32_t> hits;
  return iv_counts_back(ctx, d_hits, tiles, hits, n_hits);
}

struct HcapProbe // HcountProbe's loads; held = a member whose count lies in 1..cap
{
  HcountProbe p;
  const uint32_t* __restrict__ cnt;
  uint32_t cap;
  __device__ __forceinline__ void issue(int u, uint64_t h0) { p.issue(u, h0); }
  __device__ __forceinline__ void skip(int u) { p.skip(u); }
  __device__ __forceinline__ bool held(int u) const
  {
    const uint64_t at = p.slot(u); // (at most n_slots: the counter has n_slots + 1 counts)
    if (at == HSET_NONE) return false;
    return cnt[at] - 1u < cap; // (a count of 0 wraps to 2^32 - 1, which no cap exceeds)
  }
};

template <bool WRITE>
__global__ __launch_bounds__(HASH_THREADS) void k_hset_sample_capped(const uint8_t* __restrict__ code, const IvTile* __restrict__ tiles,
                                                                     const uint32_t* __restrict__ tile_off0, HsetView set,
                                                                     const uint32_t* __restrict__ cnt, uint32_t cap, uint64_t thresh,
                                                                     uint32_t* __restrict__ tile_cnt, const uint64_t* __restrict__ tile_at,
                                                                     SampleRec* __restrict__ out, uint64_t n_out, HashParams hp)
{
  HcapProbe probe{ HcountProbe{ HsetProbe{ set } }, cnt, cap };
  sample_tile<WRITE>(code, tiles, tile_off0, probe, thresh, tile_cnt, tile_at, out, n_out, hp);
}

// hset_sample_intervals_run with the counter beside the set: read only, `offered` stays what it is
int hset_sample_intervals_capped_run(nts_ctx* ctx, const nts_genome* g, uint32_t k, const nts_hset* s, const nts_hcount* c, uint32_t cap, uint64_t rate,
                                     const nts_interval* iv, uint64_t n_iv, uint64_t* n_sampled, nts_sample** out, uint64_t* n_out)
{
  {
    const int rc = hcount_check(ctx, s, c, 0, "nts_hset_sample_intervals_capped");
    if (rc) return rc;
  }
  const HsetView set = hset_view(s);
  const uint32_t* cnt = c->d_cnt;
  const uint8_t* code = g->d_code + PAD;
  const SampleNames nm{ "nts_hset_sample_intervals_capped", "hcount_sample_count", "hcount_sample_write", NTS_KNOB("NTS_HSET_SAMPLE_SLICE") };
  return sample_intervals_run(ctx, g, k, rate, iv, n_iv, n_sampled, out, n_out, nm,
                              [&](bool write, uint32_t n, const IvTile* d_tiles, const uint32_t* d_off0, uint64_t thresh, uint32_t* d_cnt,
                                  const uint64_t* d_at, SampleRec* d_out, uint64_t total, const HashParams& hp) {
                                if (write)
                                  NTS_LAUNCH(k_hset_sample_capped<true>, dim3(n), dim3(HASH_THREADS), 0, ctx->stream, code, d_tiles, d_off0, set, cnt, cap,
                                             thresh, d_cnt, d_at, d_out, total, hp);
                                else
                                  NTS_LAUNCH(k_hset_sample_capped<false>, dim3(n), dim3(HASH_THREADS), 0, ctx->stream, code, d_tiles, d_off0, set, cnt, cap,
                                             thresh, d_cnt, d_at, d_out, total, hp);
                              });
}

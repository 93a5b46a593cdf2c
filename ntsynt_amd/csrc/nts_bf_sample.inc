// ---- a thin sample of the k-mers of many intervals that a Bloom filter holds (nts_bf_sample_intervals; ntsynt_amd/gaps.py links) ----
// docs/design/04_10_gap_links.md.  The sibling of k_bf_count_intervals (nts_bf_iv.inc) that writes survivors instead of counting them:
// the same tiles from the same cutter and host driver (nts_iv_cut.inc), the same sweep of a tile (nts_tile_sweep.inc: this file holds
// the policy only), one workgroup per tile, a lane rolls 32 consecutive k-mers.  A k-mer survives when h0 <= UINT64_MAX / rate AND the
// filter holds it; its record is {h0, interval, offset of the k-mer from the interval's (clipped) start}.
//   two launches over the same tiles, no atomic:
//     k_bf_sample<false>  every lane gathers the survivors among its 32 k-mers as a bit mask; the workgroup adds the popcounts (wave
//                         shuffle, four partial sums through LDS) and ONE lane stores the tile's count with a plain store.  The host
//                         copies the counts back (it needs the per-interval sums anyway) and prefix-sums them into tile offsets.
//     k_bf_sample<true>   repeats the decision, finds each lane's first slot with a workgroup scan of the popcounts
//                         (block_excl_scan_256) and rolls its k-mers a second time to store the survivors' records, 16 bytes each,
//                         at tile offset + slot: k-mer order within the tile, tiles in interval order -- the output is deterministic.
//                         A lane without a survivor does not roll again; the mask is all a lane keeps between the two rolls (32
//                         hashes do not fit registers, and 8192 of them do not fit the LDS the kernel is allowed).
//   probes: only k-mers under the threshold are probed -- the index (fm), the load and the bit test all sit behind `h0 <= thresh`.
//     The batched-loads-then-test shape of the counting kernel is kept: the loads of BFS_BATCH consecutive k-mers are issued before
//     the first is looked at.  At rate 16 a lane has on average half a probe per batch of 8 in flight: the kernel is bound by the
//     hashing, not by the probes' latency, which is why the batch is not made wider than the counting kernel's.
// Experiments build only: NTS_BF_SAMPLE_SLICE = tiles per launch (default 2^23), with which the tests cut a small call into several.
// The count / write frame of a tile (sample_tile), the second roll (bfs_emit) and the host driver (sample_intervals_run) are shared with
// the sweep against a hash set (nts_hset.inc): what differs is the probe.

constexpr int BFS_BATCH = 8;

struct SampleRec // == nts_sample (include/ntsynt_hip.h)
{
  uint64_t h0;
  uint32_t iv, off;
};
static_assert(sizeof(SampleRec) == 16 && sizeof(nts_sample) == 16, "sample records are 16 bytes");

// the second roll of the write launch: the records of the k-mers in `mask`, in k-mer order, from out[0] on
template <typename BaseAt>
__device__ __forceinline__ void bfs_emit(const HashParams& hp, const uint64_t* s_tab, uint32_t mask, BaseAt&& base, uint32_t iv, uint32_t off0,
                                         SampleRec* __restrict__ out)
{
  const uint32_t last = 31u - (uint32_t)__builtin_clz(mask); // (mask != 0: the caller checks)
  uint64_t f = 0, r = 0;
  hash_init(hp, base, f, r);
  for (uint32_t j = 0;; ++j) {
    if ((mask >> j) & 1u) {
      uint4 v; // (one 16-byte store)
      const uint64_t h0 = f + r;
      v.x = (uint32_t)h0;
      v.y = (uint32_t)(h0 >> 32);
      v.z = iv;
      v.w = off0 + j;
      *reinterpret_cast<uint4*>(out++) = v;
    }
    if (j >= last) break;
    hash_roll(s_tab, base, j, hp.k, f, r);
  }
}

// What decides, beyond the threshold, whether a k-mer survives is a policy (`Probe`), so that the sweep against an exact hash set
// (nts_hset.inc) is this frame with another probe.  A probe keeps a batch's loads between issue() and held():
//   void issue(int u, uint64_t h0)   the k-mer is under the threshold: start its load(s)
//   void skip(int u)                 it is not (or it is past the lane's last): held(u) must answer false
//   bool held(int u)                 after the batch's eighth k-mer
struct BfProbe // bit h0 mod bits of a Bloom filter
{
  const uint32_t* __restrict__ bf;
  FastMod fm;
  uint32_t wd[BFS_BATCH], bit[BFS_BATCH];
  __device__ __forceinline__ void issue(int u, uint64_t h0)
  {
    const uint64_t idx = fm(h0);
    wd[u] = bf[bf_word(idx)];
    bit[u] = bf_bit(idx);
  }
  __device__ __forceinline__ void skip(int u)
  {
    wd[u] = 0;
    bit[u] = 0;
  }
  __device__ __forceinline__ bool held(int u) const { return (wd[u] >> bit[u]) & 1u; }
};

// one tile of the count (WRITE = false) or the write launch.  tile_off0[t]: offset of tile t's first k-mer from its interval's start.
// WRITE: tile_at[t] = records before tile t, n_out = records of the call (no store at or beyond it, whatever the counts say); otherwise
// tile_cnt[t] receives the tile's survivors.
template <bool WRITE, typename Probe>
__device__ __forceinline__ void sample_tile(const uint8_t* __restrict__ code, const IvTile* __restrict__ tiles, const uint32_t* __restrict__ tile_off0,
                                            Probe& probe, uint64_t thresh, uint32_t* __restrict__ tile_cnt, const uint64_t* __restrict__ tile_at,
                                            SampleRec* __restrict__ out, uint64_t n_out, const HashParams& hp)
{
  __shared__ uint64_t s_tab[36];
  __shared__ uint32_t s_seq[SEQ_LDS_DWORDS];
  __shared__ uint32_t s_w[HASH_THREADS / 64];
  const IvTile tile = tiles[blockIdx.x];
  const TileLane lane = tile_enter(s_tab, s_seq, code, tile.pos, tile.len, hp);
  // the survivors among the lane's k-mers, bit j = its j-th k-mer
  uint32_t mask = 0;
  lane.sweep(
    hp, s_tab,
    [&](uint32_t j, int u, uint64_t h0) { // (nothing is probed for a k-mer past the lane's last)
      if (j < lane.n_mine && h0 <= thresh)
        probe.issue(u, h0);
      else
        probe.skip(u);
    },
    [&](uint32_t b0) {
#pragma unroll
      for (int u = 0; u < BFS_BATCH; ++u) mask |= (uint32_t)probe.held(u) << (b0 + u);
    });
  const uint32_t mine = __popc(mask);
  if (!WRITE) {
    block_sum_store(mine, s_w, tile_cnt + blockIdx.x);
  } else {
    uint32_t total;
    const uint32_t slot = block_excl_scan_256(mine, s_w, &total);
    const uint64_t at = tile_at[blockIdx.x] + slot;
    if (mask && at + mine <= n_out) {
      const uint32_t off0 = tile_off0[blockIdx.x] + lane.first;
      if (lane.staged)
        bfs_emit(hp, s_tab, mask, lane.lds, tile.iv, off0, out + at);
      else
        bfs_emit(hp, s_tab, mask, lane.mem, tile.iv, off0, out + at);
    }
  }
}

template <bool WRITE>
__global__ __launch_bounds__(HASH_THREADS) void k_bf_sample(const uint8_t* __restrict__ code, const IvTile* __restrict__ tiles,
                                                            const uint32_t* __restrict__ tile_off0, const uint32_t* __restrict__ bf, FastMod fm,
                                                            uint64_t thresh, uint32_t* __restrict__ tile_cnt, const uint64_t* __restrict__ tile_at,
                                                            SampleRec* __restrict__ out, uint64_t n_out, HashParams hp)
{
  BfProbe probe{ bf, fm };
  sample_tile<WRITE>(code, tiles, tile_off0, probe, thresh, tile_cnt, tile_at, out, n_out, hp);
}

// what a sampling call is named by: its C name, its two timers, its experiments-build knob
struct SampleNames
{
  const char *who, *timer_count, *timer_write, *knob;
};

// the host side of a sampling sweep: tiles, count launch, prefix sums, write launch, records to the host.  launch(write, n, d_tiles, d_off0,
// thresh, d_cnt, d_at, d_out, total, hp) starts one launch over n tiles (the per-tile pointers already point at the first of them).
template <typename Launch>
int sample_intervals_run(nts_ctx* ctx, const nts_genome* g, uint32_t k, uint64_t rate, const nts_interval* iv, uint64_t n_iv, uint64_t* n_sampled,
                         nts_sample** out, uint64_t* n_out, const SampleNames& nm, Launch&& launch)
{
  const std::string who = nm.who;
  *out = nullptr;
  *n_out = 0;
  if (n_iv == 0) return NTS_OK;
  std::vector<uint64_t> nk;
  std::vector<IvTile> tiles;
  HashParams hp;
  {
    const int rc = iv_cut_tiles(ctx, g, k, iv, n_iv, nm.who, nk, tiles, &hp);
    if (rc) return rc;
  }
  std::vector<uint64_t> iv_a(n_iv); // the intervals' (clipped) starts, as iv_cut_pieces clips
  for (uint64_t i = 0; i < n_iv; ++i) {
    n_sampled[i] = 0;
    const uint64_t len = g->rec_len[iv[i].rec];
    const uint64_t a = g->rec_off[iv[i].rec] + std::min(iv[i].start, len), b = g->rec_off[iv[i].rec] + std::min(iv[i].end, len);
    if (b > a && b - a > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, who + ": an interval of 2^32 bases or more (offsets are 32-bit)");
    iv_a[i] = a;
  }
  if (tiles.empty()) return NTS_OK;
  std::vector<uint32_t> off0(tiles.size());
  for (size_t t = 0; t < tiles.size(); ++t) off0[t] = (uint32_t)(tiles[t].pos - iv_a[tiles[t].iv]);
  const uint64_t thresh = ~0ULL / rate;
  const size_t nt = tiles.size();
  NTS_WS(d_cnt, uint32_t*, "bfs_cnt", nt * 4); // (before the uploads: nothing may fail between an asynchronous copy out of a host vector and the synchronise behind it)
  NTS_WS(d_at, uint64_t*, "bfs_at", nt * 8);
  IvTile* d_tiles = nullptr;
  uint32_t* d_off0 = nullptr;
  {
    int rc = ws_upload(ctx, "bfs_tiles", tiles, &d_tiles);
    if (rc == NTS_OK) rc = ws_upload(ctx, "bfs_off0", off0, &d_off0);
    if (rc) {
      hipStreamSynchronize(ctx->stream);
      return rc;
    }
  }
  const uint64_t slice = iv_slice(nm.knob);
  iv_for_slices(ctx, nm.timer_count, nt, slice, [&](uint64_t t0, uint32_t n) {
    launch(false, n, d_tiles + t0, d_off0 + t0, thresh, d_cnt + t0, (const uint64_t*)nullptr, (SampleRec*)nullptr, (uint64_t)0, hp);
  });
  std::vector<uint32_t> cnt;
  {
    const int rc = iv_counts_back(ctx, d_cnt, tiles, cnt, n_sampled);
    if (rc) return rc;
  }
  std::vector<uint64_t> at(nt);
  uint64_t total = 0;
  for (size_t t = 0; t < nt; ++t) {
    at[t] = total;
    total += cnt[t];
  }
  if (total > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, who + ": 2^32 records or more (raise the rate or pass fewer intervals)");
  if (total == 0) return NTS_OK;
  NTS_WS(d_out, SampleRec*, "bfs_out", total * sizeof(SampleRec));
  nts_sample* host = (nts_sample*)malloc(total * sizeof(nts_sample));
  if (!host) return fail(ctx, NTS_ENOMEM, who + ": host memory for the records");
  hipError_t e = hipMemcpyAsync(d_at, at.data(), nt * 8, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    iv_for_slices(ctx, nm.timer_write, nt, slice, [&](uint64_t t0, uint32_t n) {
      launch(true, n, d_tiles + t0, d_off0 + t0, thresh, (uint32_t*)nullptr, (const uint64_t*)(d_at + t0), d_out, total, hp);
    });
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(host, d_out, total * sizeof(SampleRec), hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t e_sync = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess || e_sync != hipSuccess) free(host);
  HIP_TRY(ctx, e);
  HIP_TRY(ctx, e_sync);
  *out = host;
  *n_out = total;
  return NTS_OK;
}

int bf_sample_intervals_run(nts_ctx* ctx, const nts_genome* g, uint32_t k, const nts_bf* bf, uint64_t rate, const nts_interval* iv,
                            uint64_t n_iv, uint64_t* n_sampled, nts_sample** out, uint64_t* n_out)
{
  const FastMod fm = make_fastmod(bf->bytes * 8);
  const uint8_t* code = g->d_code + PAD;
  const SampleNames nm{ "nts_bf_sample_intervals", "bf_sample_count", "bf_sample_write", NTS_KNOB("NTS_BF_SAMPLE_SLICE") };
  return sample_intervals_run(ctx, g, k, rate, iv, n_iv, n_sampled, out, n_out, nm,
                              [&](bool write, uint32_t n, const IvTile* d_tiles, const uint32_t* d_off0, uint64_t thresh, uint32_t* d_cnt,
                                  const uint64_t* d_at, SampleRec* d_out, uint64_t total, const HashParams& hp) {
                                if (write)
                                  NTS_LAUNCH(k_bf_sample<true>, dim3(n), dim3(HASH_THREADS), 0, ctx->stream, code, d_tiles, d_off0, bf->d_words, fm, thresh,
                                             d_cnt, d_at, d_out, total, hp);
                                else
                                  NTS_LAUNCH(k_bf_sample<false>, dim3(n), dim3(HASH_THREADS), 0, ctx->stream, code, d_tiles, d_off0, bf->d_words, fm, thresh,
                                             d_cnt, d_at, d_out, total, hp);
                              });
}

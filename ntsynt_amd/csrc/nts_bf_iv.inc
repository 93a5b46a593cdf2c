// ---- how many k-mers of each of many intervals a Bloom filter holds (nts_bf_count_intervals; ntsynt_amd/gaps.py) -------------------
// docs/design/04_9_gap_content.md.  The intervals are cut into tiles of valid k-mers on the host (nts_iv_cut.inc: n_kmers[i] falls out
// of it); one workgroup sweeps one tile (nts_tile_sweep.inc: this file holds the policy only) and probes the filter once per k-mer, as
// k_hash<MODE_KEYS> does -- the index is fm(h0), word and bit are bf_test's (bf_word / bf_bit, nts_device.h) -- but nothing is written per k-mer: a lane counts its hits in a
// register, the workgroup adds them up (wave shuffle, four partial sums through LDS) and ONE lane stores the tile's count with a plain
// store.  The host adds the tiles of an interval.  No atomic anywhere: intervals may overlap and come in any order, every tile has a
// slot of its own.
//   probes in flight: BFI_BATCH = 8 independent 4-byte loads per lane are issued before the first is looked at, as in
//        k_hash<MODE_KEYS>.  The kernel is bound by the latency of those loads -- every one a miss of a filter far larger than the
//        caches -- so what counts is waves x probes in flight: with 8 the kernel takes 59 vector registers, eight waves per SIMD (the
//        9.9 KB of LDS per workgroup allow sixteen workgroups per CU, twice that) = 64 probes per SIMD lane; a batch of 16 takes 86
//        registers, five waves = 80 probes, and forced into 64 registers it spills (tests/test_bf_iv_isa_guard.py holds the 64).
//   k > FAST_K_MAX: the sweep's per-lane loads, with the same batches of 8 probes.
// Experiments build only: NTS_BF_IV_SLICE = tiles per launch (default 2^23), with which the tests cut a small call into several.

constexpr int BFI_BATCH = 8;

__global__ __launch_bounds__(HASH_THREADS) void k_bf_count_intervals(const uint8_t* __restrict__ code, const IvTile* __restrict__ tiles,
                                                                     const uint32_t* __restrict__ bf, FastMod fm, uint32_t* __restrict__ tile_hits,
                                                                     HashParams hp)
{
  __shared__ uint64_t s_tab[36];
  __shared__ uint32_t s_seq[SEQ_LDS_DWORDS];
  __shared__ uint32_t s_hits[HASH_THREADS / 64];
  const IvTile tile = tiles[blockIdx.x];
  const TileLane lane = tile_enter(s_tab, s_seq, code, tile.pos, tile.len, hp);
  uint32_t hits = 0;
  uint32_t wd[BFI_BATCH], bit[BFI_BATCH];
  lane.sweep(
    hp, s_tab,
    [&](uint32_t j, int u, uint64_t h) { // (bf_test in two halves: the load now, the bit after the batch's loads are out; a k-mer past the lane's last reads word 0)
      const bool live = j < lane.n_mine;
      const uint64_t idx = fm(h);
      wd[u] = bf[live ? bf_word(idx) : 0ULL];
      bit[u] = live ? bf_bit(idx) : 32u;
    },
    [&](uint32_t) {
#pragma unroll
      for (int u = 0; u < BFI_BATCH; ++u) hits += bit[u] != 32u ? (wd[u] >> bit[u]) & 1u : 0u;
    });
  block_sum_store(hits, s_hits, tile_hits + blockIdx.x);
}

int bf_count_intervals_run(nts_ctx* ctx, const nts_genome* g, uint32_t k, const nts_bf* bf, const nts_interval* iv, uint64_t n_iv,
                           uint64_t* n_kmers, uint64_t* n_hits)
{
  if (n_iv == 0) return NTS_OK;
  std::vector<uint64_t> nk;
  std::vector<IvTile> tiles;
  HashParams hp;
  {
    const int rc = iv_cut_tiles(ctx, g, k, iv, n_iv, "nts_bf_count_intervals", nk, tiles, &hp);
    if (rc) return rc;
  }
  for (uint64_t i = 0; i < n_iv; ++i) {
    n_kmers[i] = nk[i];
    n_hits[i] = 0;
  }
  if (tiles.empty()) return NTS_OK;
  const FastMod fm = make_fastmod(bf->bytes * 8);
  NTS_WS(d_hits, uint32_t*, "bfi_hits", tiles.size() * 4); // (before the upload: nothing may fail between the asynchronous copy out of `tiles` and the synchronise of iv_counts_back)
  IvTile* d_tiles = nullptr;
  {
    const int rc = ws_upload(ctx, "bfi_tiles", tiles, &d_tiles);
    if (rc) return rc;
  }
  iv_for_slices(ctx, "bf_count_iv", tiles.size(), iv_slice(NTS_KNOB("NTS_BF_IV_SLICE")), [&](uint64_t t0, uint32_t nt) {
    NTS_LAUNCH(k_bf_count_intervals, dim3(nt), dim3(HASH_THREADS), 0, ctx->stream, g->d_code + PAD, d_tiles + t0, bf->d_words, fm, d_hits + t0, hp);
  });
  std::vector<uint32_t> hits;
  return iv_counts_back(ctx, d_hits, tiles, hits, n_hits);
}

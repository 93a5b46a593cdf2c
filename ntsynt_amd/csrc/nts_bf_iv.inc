// ---- how many k-mers of each of many intervals a Bloom filter holds (nts_bf_count_intervals; ntsynt_amd/gaps.py) -------------------
// docs/design/04_9_gap_content.md.  The intervals are cut into tiles of valid k-mers on the host (nts_iv_cut.inc: n_kmers[i] falls out
// of it); one workgroup hashes one tile the way k_hash's fast path does and probes the filter once per k-mer, as k_hash<MODE_KEYS>
// does -- the index is fm(h0), word and bit are bf_test's (bf_word / bf_bit, nts_device.h) -- but nothing is written per k-mer: a lane counts its hits in a
// register, the workgroup adds them up (wave shuffle, four partial sums through LDS) and ONE lane stores the tile's count with a plain
// store.  The host adds the tiles of an interval.  No atomic anywhere: intervals may overlap and come in any order, every tile has a
// slot of its own.
//   probes in flight: BFI_BATCH = 8 independent 4-byte loads per lane are issued before the first is looked at, as in
//        k_hash<MODE_KEYS>.  The kernel is bound by the latency of those loads -- every one a miss of a filter far larger than the
//        caches -- so what counts is waves x probes in flight: with 8 the kernel takes 60 vector registers, eight waves per SIMD (the
//        9.9 KB of LDS per workgroup allow sixteen workgroups per CU, twice that) = 64 probes per SIMD lane; a batch of 16 takes 86
//        registers, five waves = 80 probes, and forced into 64 registers it spills (tests/test_bf_iv_isa_guard.py holds the 64).
//   k > FAST_K_MAX: the bases do not fit the staging area; every lane reads its own from the L2 (the tile lies inside one stretch of
//        valid bases, so positions are plain offsets), as in k_minhash_intervals.
// Experiments build only: NTS_BF_IV_SLICE = tiles per launch (default 2^23), with which the tests cut a small call into several.

constexpr int BFI_BATCH = 8;

__global__ __launch_bounds__(HASH_THREADS) void k_bf_count_intervals(const uint8_t* __restrict__ code, const IvTile* __restrict__ tiles,
                                                                     const uint32_t* __restrict__ bf, FastMod fm, uint32_t* __restrict__ tile_hits,
                                                                     HashParams hp)
{
  __shared__ uint64_t s_tab[36];
  __shared__ uint32_t s_seq[SEQ_LDS_DWORDS];
  __shared__ uint32_t s_hits[HASH_THREADS / 64];
  const uint32_t tid = threadIdx.x;
  if (tid < 16) {
    s_tab[tid] = hp.roll_f[tid];
    s_tab[16 + tid] = hp.roll_r[tid];
  }
  if (tid < 4) s_tab[32 + tid] = hp.seed[tid];
  const uint32_t k = hp.k;
  const IvTile tile = tiles[blockIdx.x];
  const uint32_t tile_len = min(tile.len, KEY_TILE);
  const uint32_t first = 32u * tid;
  const uint32_t n_mine = first < tile_len ? min(32u, tile_len - first) : 0u;
  uint32_t hits = 0;
  if (k > FAST_K_MAX) {
    __syncthreads();
    if (n_mine) {
      const uint8_t* p = code + tile.pos + first;
      uint64_t f = 0, r = 0;
      hash_init(hp, [&](uint32_t i) -> uint32_t { return p[i] & 3u; }, f, r);
      for (uint32_t i = 0;;) {
        hits += bf_test(bf, fm(f + r)) ? 1u : 0u;
        if (++i >= n_mine) break;
        const uint32_t cout = p[0] & 3u, cin = p[k] & 3u;
        f = srol1(f) ^ s_tab[cin * 4 + cout];
        r = sror1(r ^ s_tab[16 + cin * 4 + cout]);
        ++p;
      }
    }
  } else {
    // ---- the tile's bases into LDS: 16-byte loads, 4 bytes of padding per 32 (lane stride 36 B: conflict-free byte reads)
    const uint32_t a = (uint32_t)(tile.pos & 15u);
    const uint8_t* src = code + (tile.pos - a);
    const uint32_t n_bytes = a + tile_len + k - 1;
    const uint32_t n16 = (n_bytes + 15u) >> 4;
    for (uint32_t c = tid; c < n16; c += HASH_THREADS) {
      const uint4 v = *reinterpret_cast<const uint4*>(src + 16u * c);
      const uint32_t d = 4u * c + (c >> 1);
      s_seq[d] = v.x;
      s_seq[d + 1] = v.y;
      s_seq[d + 2] = v.z;
      s_seq[d + 3] = v.w;
    }
    __syncthreads();
    const uint8_t* sb = reinterpret_cast<const uint8_t*>(s_seq);
    auto base_at = [&](uint32_t s) -> uint32_t { return sb[s + 4u * (s >> 5)] & 3u; };
    uint32_t s = a + first;
    uint64_t f = 0, r = 0;
    if (n_mine) hash_init(hp, [&](uint32_t i) { return base_at(s + i); }, f, r);
#pragma unroll 1
    for (uint32_t b0 = 0; b0 < 32; b0 += BFI_BATCH) {
      if (b0 >= n_mine) break;
      uint32_t wd[BFI_BATCH], bit[BFI_BATCH];
#pragma unroll
      for (int u = 0; u < BFI_BATCH; ++u) { // (a lane with fewer than 32 k-mers rolls on inside the staging area and reads word 0 for those)
        const bool live = b0 + u < n_mine;
        const uint64_t idx = fm(f + r);
        wd[u] = bf[live ? bf_word(idx) : 0ULL]; // (bf_test in two halves: the load now, the bit after the batch's loads are out)
        bit[u] = live ? bf_bit(idx) : 32u;
        const uint32_t cout = base_at(s), cin = base_at(s + k);
        f = srol1(f) ^ s_tab[cin * 4 + cout];
        r = sror1(r ^ s_tab[16 + cin * 4 + cout]);
        ++s;
      }
#pragma unroll
      for (int u = 0; u < BFI_BATCH; ++u) hits += bit[u] != 32u ? (wd[u] >> bit[u]) & 1u : 0u;
    }
  }
  // ---- the tile's hits: lanes -> wave -> workgroup, one plain store
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) hits += __shfl_down(hits, d, 64);
  if ((tid & 63u) == 0) s_hits[tid >> 6] = hits;
  __syncthreads();
  if (tid == 0) {
    uint32_t sum = 0;
#pragma unroll
    for (int wv = 0; wv < HASH_THREADS / 64; ++wv) sum += s_hits[wv];
    tile_hits[blockIdx.x] = sum;
  }
}

int bf_count_intervals_run(nts_ctx* ctx, const nts_genome* g, uint32_t k, const nts_bf* bf, const nts_interval* iv, uint64_t n_iv,
                           uint64_t* n_kmers, uint64_t* n_hits)
{
  if (n_iv == 0) return NTS_OK;
  std::vector<IvPiece> pieces;
  std::vector<uint64_t> piece_at, nk;
  {
    const int rc = iv_cut_pieces(ctx, g, k, iv, n_iv, "nts_bf_count_intervals", pieces, piece_at, nk);
    if (rc) return rc;
  }
  if (n_iv > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_bf_count_intervals: more than 2^32 - 1 intervals in one call");
  std::vector<IvTile> tiles;
  for (uint64_t i = 0; i < n_iv; ++i) {
    n_kmers[i] = nk[i];
    n_hits[i] = 0;
    iv_append_tiles(pieces, piece_at, i, (uint32_t)i, tiles);
  }
  if (tiles.empty()) return NTS_OK;
  HashParams hp;
  {
    const int rc = hash_params_for(ctx, k, &hp);
    if (rc) return rc;
  }
  const FastMod fm = make_fastmod(bf->bytes * 8);
  NTS_WS(d_hits, uint32_t*, "bfi_hits", tiles.size() * 4); // (before the upload: nothing may fail between the asynchronous copy out of `tiles` and the synchronise below)
  IvTile* d_tiles = nullptr;
  {
    const int rc = ws_upload(ctx, "bfi_tiles", tiles, &d_tiles);
    if (rc) return rc;
  }
  uint64_t slice = (uint64_t)1 << 23; // tiles per launch: 2^31 work-items
  if (const char* v = NTS_KNOB("NTS_BF_IV_SLICE")) slice = std::min<uint64_t>(std::max<uint64_t>(strtoull(v, nullptr, 0), 1), slice);
  for (uint64_t t0 = 0; t0 < tiles.size(); t0 += slice) {
    const uint32_t nt = (uint32_t)std::min<uint64_t>(slice, tiles.size() - t0);
    ScopedTimer t(ctx, "bf_count_iv", true);
    NTS_LAUNCH(k_bf_count_intervals, dim3(nt), dim3(HASH_THREADS), 0, ctx->stream, g->d_code + PAD, d_tiles + t0, bf->d_words, fm, d_hits + t0, hp);
  }
  std::vector<uint32_t> hits(tiles.size());
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(hits.data(), d_hits, tiles.size() * 4, hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t e_sync = hipStreamSynchronize(ctx->stream); // (whatever happened: `tiles` and `hits` are read and written by asynchronous copies)
  HIP_TRY(ctx, e);
  HIP_TRY(ctx, e_sync);
  for (size_t t = 0; t < tiles.size(); ++t) n_hits[tiles[t].iv] += hits[t];
  return NTS_OK;
}

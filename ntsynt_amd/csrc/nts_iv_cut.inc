// ---- intervals of a resident genome -> tiles of valid k-mers, and the host side of a sweep over them --------------------------------
// (nts_minhash_intervals, nts_bf_count_intervals, nts_bf_sample_intervals)
// The host cuts each interval against the genome's stretches of valid bases (nts_genome::st_a / st_b) into pieces of at least k bases,
// and the pieces into tiles of at most KEY_TILE k-mers: every k-mer of a tile is valid, lies wholly inside its interval, and the
// tile's bases are contiguous -- so one workgroup sweeps one tile (nts_tile_sweep.inc) and needs no run table.  The k-mers of an
// interval fall out of the cutting.  [start, end) is clipped to the record; an interval shorter than k, empty or inside N has no piece.
// A sweep is launched over at most 2^23 tiles at a time (iv_for_slices); where every tile leaves a count in a slot of its own, the
// host fetches the slots and adds up the tiles of each interval (iv_counts_back).

struct IvPiece
{
  uint64_t pos, nk; // index into the genome's codes of the piece's first k-mer; its k-mers
};

struct IvTile
{
  uint64_t pos; // index into the genome's codes of the tile's first k-mer
  uint32_t iv;  // interval (within the chunk: nts_minhash_intervals; of the call: iv_cut_tiles)
  uint32_t len; // k-mers, 1 .. KEY_TILE
};

// pieces[piece_at[i] .. piece_at[i + 1]) are interval i's runs of k-mers, nk[i] their sum.  `who`: the call, for the message.
int iv_cut_pieces(nts_ctx* ctx, const nts_genome* g, uint32_t k, const nts_interval* iv, uint64_t n_iv, const char* who,
                  std::vector<IvPiece>& pieces, std::vector<uint64_t>& piece_at, std::vector<uint64_t>& nk)
{
  pieces.clear();
  piece_at.assign(n_iv + 1, 0);
  nk.assign(n_iv, 0);
  const size_t ns = g->st_a.size();
  for (uint64_t i = 0; i < n_iv; ++i) {
    if (iv[i].rec >= g->n_rec) return fail(ctx, NTS_EINVAL, std::string(who) + ": record index out of range");
    const uint64_t len = g->rec_len[iv[i].rec];
    const uint64_t a = g->rec_off[iv[i].rec] + std::min(iv[i].start, len), b = g->rec_off[iv[i].rec] + std::min(iv[i].end, len);
    if (b > a && b - a >= k) {
      size_t q = (size_t)(std::upper_bound(g->st_b.begin(), g->st_b.end(), a) - g->st_b.begin()); // first stretch that ends behind a
      for (; q < ns && g->st_a[q] < b; ++q) {
        const uint64_t pa = std::max(a, g->st_a[q]), pb = std::min(b, g->st_b[q]);
        if (pb > pa && pb - pa >= k) {
          pieces.push_back({ pa, pb - pa - k + 1 });
          nk[i] += pb - pa - k + 1;
        }
      }
    }
    piece_at[i + 1] = pieces.size();
  }
  return NTS_OK;
}

// the tiles of interval i, numbered `id`, behind those in `tiles`
inline void iv_append_tiles(const std::vector<IvPiece>& pieces, const std::vector<uint64_t>& piece_at, uint64_t i, uint32_t id,
                            std::vector<IvTile>& tiles)
{
  for (uint64_t q = piece_at[i]; q < piece_at[i + 1]; ++q)
    for (uint64_t at = 0; at < pieces[q].nk; at += KEY_TILE)
      tiles.push_back({ pieces[q].pos + at, id, (uint32_t)std::min<uint64_t>(KEY_TILE, pieces[q].nk - at) });
}

// a whole call at once: nk[i] = the k-mers of interval i, tiles = those of all intervals in order, numbered by interval; hp for k
// (not set when there is no tile)
int iv_cut_tiles(nts_ctx* ctx, const nts_genome* g, uint32_t k, const nts_interval* iv, uint64_t n_iv, const char* who, std::vector<uint64_t>& nk,
                 std::vector<IvTile>& tiles, HashParams* hp)
{
  std::vector<IvPiece> pieces;
  std::vector<uint64_t> piece_at;
  {
    const int rc = iv_cut_pieces(ctx, g, k, iv, n_iv, who, pieces, piece_at, nk);
    if (rc) return rc;
  }
  if (n_iv > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, std::string(who) + ": more than 2^32 - 1 intervals in one call");
  tiles.clear();
  for (uint64_t i = 0; i < n_iv; ++i) iv_append_tiles(pieces, piece_at, i, (uint32_t)i, tiles);
  return tiles.empty() ? NTS_OK : hash_params_for(ctx, k, hp);
}

// tiles per launch: 2^23 (2^31 work-items), or what an experiments-build knob asks for, 1 .. 2^23 (`knob`: its value or nullptr)
inline uint64_t iv_slice(const char* knob)
{
  const uint64_t most = (uint64_t)1 << 23;
  return knob ? std::min<uint64_t>(std::max<uint64_t>(strtoull(knob, nullptr, 0), 1), most) : most;
}

// launch(t0, n) for tiles [t0, t0 + n), slice after slice, each under the timer `timer`
template <typename Launch>
void iv_for_slices(nts_ctx* ctx, const char* timer, uint64_t n_tiles, uint64_t slice, Launch&& launch)
{
  for (uint64_t t0 = 0; t0 < n_tiles; t0 += slice) {
    ScopedTimer t(ctx, timer, true);
    launch(t0, (uint32_t)std::min<uint64_t>(slice, n_tiles - t0));
  }
}

// behind the launches of a counting sweep: cnt = the tiles' counts, copied back; sum[tile.iv] += each.  The stream is synchronised
// whatever happened: host vectors (the tiles, cnt) are read and written by asynchronous copies.
int iv_counts_back(nts_ctx* ctx, const uint32_t* d_cnt, const std::vector<IvTile>& tiles, std::vector<uint32_t>& cnt, uint64_t* sum)
{
  cnt.resize(tiles.size());
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(cnt.data(), d_cnt, tiles.size() * 4, hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t e_sync = hipStreamSynchronize(ctx->stream);
  HIP_TRY(ctx, e);
  HIP_TRY(ctx, e_sync);
  for (size_t t = 0; t < tiles.size(); ++t) sum[tiles[t].iv] += cnt[t];
  return NTS_OK;
}

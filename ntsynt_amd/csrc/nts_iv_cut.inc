// ---- intervals of a resident genome -> tiles of valid k-mers (nts_minhash_intervals, nts_bf_count_intervals) ------------------------
// The host cuts each interval against the genome's stretches of valid bases (nts_genome::st_a / st_b) into pieces of at least k bases,
// and the pieces into tiles of at most KEY_TILE k-mers: every k-mer of a tile is valid, lies wholly inside its interval, and the
// tile's bases are contiguous -- so a workgroup does what k_hash's fast path does (bases staged through LDS with 16-byte loads, each
// lane hashes its first k-mer from the init table and rolls 31 times) and needs no run table.  The k-mers of an interval fall out of
// the cutting.  [start, end) is clipped to the record; an interval shorter than k, empty or inside N has no piece.

struct IvPiece
{
  uint64_t pos, nk; // index into the genome's codes of the piece's first k-mer; its k-mers
};

struct IvTile
{
  uint64_t pos; // index into the genome's codes of the tile's first k-mer
  uint32_t iv;  // interval (within the chunk: nts_minhash_intervals; of the call: nts_bf_count_intervals)
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

// ---- a thin sample of the k-mers of many intervals, whatever holds them (nts_sample_intervals; ntsynt_amd/gaps.py sample_all, periods) ----
// docs/design/04_14_gap_periods.md.  nts_bf_sample_intervals without the filter: the same tiles, the same frame of a tile (sample_tile:
// count launch, write launch, no atomic), the same second roll (bfs_emit) and host driver (sample_intervals_run) -- this file brings the
// probe only.  A k-mer survives when h0 <= UINT64_MAX / rate; sample_tile tests that (and `j < n_mine`) before it calls issue(), so the
// probe has nothing to look up: issue records a bit, skip clears it, held returns it.  No index, no load, no arrays per batch: one
// 32-bit mask of which the batch's eight bits are used.  What a tandem array's k-mers need: an array that one genome alone has is in
// no common filter and in no set built from a filter-gated sample.
// Experiments build only: NTS_IV_SAMPLE_SLICE = tiles per launch (default 2^23), as NTS_BF_SAMPLE_SLICE.

struct NoProbe // under the threshold = held
{
  uint32_t bits;
  __device__ __forceinline__ void issue(int u, uint64_t) { bits |= 1u << u; }
  __device__ __forceinline__ void skip(int u) { bits &= ~(1u << u); }
  __device__ __forceinline__ bool held(int u) const { return (bits >> u) & 1u; }
};

template <bool WRITE>
__global__ __launch_bounds__(HASH_THREADS) void k_iv_sample(const uint8_t* __restrict__ code, const IvTile* __restrict__ tiles,
                                                            const uint32_t* __restrict__ tile_off0, uint64_t thresh, uint32_t* __restrict__ tile_cnt,
                                                            const uint64_t* __restrict__ tile_at, SampleRec* __restrict__ out, uint64_t n_out,
                                                            HashParams hp)
{
  NoProbe probe{ 0u };
  sample_tile<WRITE>(code, tiles, tile_off0, probe, thresh, tile_cnt, tile_at, out, n_out, hp);
}

int iv_sample_intervals_run(nts_ctx* ctx, const nts_genome* g, uint32_t k, uint64_t rate, const nts_interval* iv, uint64_t n_iv, uint64_t* n_sampled,
                            nts_sample** out, uint64_t* n_out)
{
  const uint8_t* code = g->d_code + PAD;
  const SampleNames nm{ "nts_sample_intervals", "iv_sample_count", "iv_sample_write", NTS_KNOB("NTS_IV_SAMPLE_SLICE") };
  return sample_intervals_run(ctx, g, k, rate, iv, n_iv, n_sampled, out, n_out, nm,
                              [&](bool write, uint32_t n, const IvTile* d_tiles, const uint32_t* d_off0, uint64_t thresh, uint32_t* d_cnt,
                                  const uint64_t* d_at, SampleRec* d_out, uint64_t total, const HashParams& hp) {
                                if (write)
                                  NTS_LAUNCH(k_iv_sample<true>, dim3(n), dim3(HASH_THREADS), 0, ctx->stream, code, d_tiles, d_off0, thresh, d_cnt, d_at, d_out,
                                             total, hp);
                                else
                                  NTS_LAUNCH(k_iv_sample<false>, dim3(n), dim3(HASH_THREADS), 0, ctx->stream, code, d_tiles, d_off0, thresh, d_cnt, d_at, d_out,
                                             total, hp);
                              });
}

// ---- the exact edit distance of the two strings of every candidate segment, summed per interval (nts_edit_segments; ----
// ntsynt_amd/assess.py block_identity).  docs/design/04_16_block_identity.md.  A segment (nts_iv_anchor_segments) names dx bases of an
// interval of genome A and dy bases of its mate in genome B, the latter reverse-complemented where the pair is flipped.  Unit-cost
// Levenshtein distance restricted to the diagonals -W .. W; the result D is accepted when (D + |dy - dx|) / 2 <= W, which is exactly
// when the unrestricted distance satisfies the same inequality, and then the two are equal.
// k_edit_wave: one 64-lane wave per segment, EDIT_WAVES waves per workgroup.  Lane l owns the diagonal d = l - W (d = j - i: i bases of
// A against j bases of B) and keeps that diagonal's last value in a register.  The wave steps over the antidiagonals t = i + j; on
// step t the lanes with t - d even own a cell (i, j) = ((t - d) / 2, (t + d) / 2) and take
//   min(own value, two steps old, + (A[i - 1] != B[j - 1]);  left neighbour's + 1 = cell (i, j - 1);  right neighbour's + 1 = cell (i - 1, j))
// A register starts at EDIT_INF (0 on diagonal 0) and is written only for cells inside the matrix, so a neighbour whose cell would lie
// outside it (i - 1 < 0, j - 1 < 0) or outside the band still holds EDIT_INF; every sum is clamped to EDIT_INF (saturating, no wrap).
// The bases come through LDS: per EDIT_CHUNK antidiagonals the wave stages the EDIT_WIN bases of each string that those steps can
// touch, with coalesced byte loads, B read backwards and complemented where the pair is flipped.  Only positions inside the two
// strings are loaded (a string lies inside its interval, an interval inside its record: checked on the host and again per lane), every
// position of either string is staged by some chunk, and a code >= CODE_INVALID seen while staging makes the segment `invalid`.
// The inner loop reads two LDS bytes and exchanges two registers across lanes; it issues no global load.
// k_edit_kinds + one rocprim::reduce_by_key over iv_a give the sums per interval (segments arrive in iv_a order), k_edit_store puts
// them at out[iv_a].  No atomic, no launch per segment, no floating point.

constexpr uint32_t EDIT_INF = 0x3FFFFFFFu;
constexpr uint32_t EDIT_WAVES = 4;
constexpr uint32_t EDIT_CHUNK = 256; // antidiagonals per staging
constexpr uint32_t EDIT_WIN = 192;   // bases of each string staged per chunk: EDIT_CHUNK / 2 + W + 2 <= 161 at W = 31, three per lane
constexpr uint32_t EDIT_MAX_BAND = 31, EDIT_MAX_LEN = 65535;
static_assert(2 * EDIT_MAX_BAND + 1 <= 63, "lane 63 is never a diagonal of the band: the right neighbour of the last one holds EDIT_INF");
static_assert(EDIT_CHUNK / 2 + EDIT_MAX_BAND + 2 <= EDIT_WIN && EDIT_WIN % 64 == 0, "the staged window holds every base a chunk can touch");
static_assert(sizeof(nts_iv_identity) == 56, "the C ABI's layout");

struct EditIv // what the kernel needs of an interval of A and its mate
{
  uint64_t a0, b0; // index into the genomes' codes of the two clipped starts
  uint32_t la, lb; // clipped lengths
  uint32_t flip, pad;
};

struct EditAdd
{
  __host__ __device__ nts_iv_identity operator()(const nts_iv_identity& x, const nts_iv_identity& y) const
  {
    return { x.aligned_a + y.aligned_a, x.aligned_b + y.aligned_b, x.edits + y.edits, x.segments + y.segments, x.aligned + y.aligned,
             x.backward + y.backward,   x.too_long + y.too_long,   x.offband + y.offband, x.invalid + y.invalid, x.overband + y.overband, 0u };
  }
};

struct EditIvOf
{
  __host__ __device__ uint32_t operator()(const nts_iv_segment& s) const { return s.iv_a; }
};

__global__ __launch_bounds__(EDIT_WAVES * 64) void k_edit_wave(const uint8_t* __restrict__ code_a, const uint8_t* __restrict__ code_b,
                                                               const EditIv* __restrict__ ivs, uint64_t n_iv, const nts_iv_segment* __restrict__ segs,
                                                               uint64_t n_segs, uint32_t W, uint32_t* __restrict__ dist)
{
  __shared__ uint8_t s_a[EDIT_WAVES][EDIT_WIN], s_b[EDIT_WAVES][EDIT_WIN];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t sidx = (uint64_t)blockIdx.x * EDIT_WAVES + wv;
  if (sidx >= n_segs) return;
  const nts_iv_segment s = segs[sidx];
  if (s.kind != NTS_SEG_CANDIDATE) {
    if (lane == 0) dist[sidx] = s.kind <= NTS_SEG_OFFBAND ? NTS_EDIT_PASSED : NTS_EDIT_NOT_CANDIDATE;
    return;
  }
  const int dx = (int)s.dx, dy = s.dy;
  const int delta = dy - dx, ad = delta < 0 ? -delta : delta;
  EditIv v{ 0, 0, 0, 0, 0, 0 };
  if (s.iv_a < n_iv) v = ivs[s.iv_a];
  // (the host refused all of this before the launch: a lane still loads nothing outside its two strings' intervals)
  if (W < 1 || W > EDIT_MAX_BAND || dx < 1 || dy < 1 || dx > (int)EDIT_MAX_LEN || dy > (int)EDIT_MAX_LEN || ad > (int)W || (uint64_t)s.x + (uint32_t)dx > v.la ||
      (uint64_t)s.y_lo + (uint32_t)dy > v.lb) {
    if (lane == 0) dist[sidx] = NTS_EDIT_NOT_CANDIDATE;
    return;
  }
  const uint8_t* const pa = code_a + v.a0 + s.x;
  const bool flip = v.flip != 0;
  // B[q] of the oriented string: forwards from y_lo, or backwards from the base that mirrors y_lo, complemented
  const uint8_t* const pb = flip ? code_b + v.b0 + (v.lb - 1u - s.y_lo) : code_b + v.b0 + s.y_lo;
  const int d = (int)lane - (int)W;
  const bool in_band = lane <= 2u * W;
  uint32_t val = lane == W ? 0u : EDIT_INF;
  bool bad = false;
  const int T = dx + dy;
  for (int t0 = 1; t0 <= T; t0 += (int)EDIT_CHUNK) {
    // the chunk's cells have i - 1 and j - 1 in [lo, lo + EDIT_WIN): (t -/+ d) / 2 - 1 with |d| <= W, t0 <= t < t0 + EDIT_CHUNK
    const int lo = ((t0 - (int)W) >> 1) - 1;
#pragma unroll
    for (uint32_t q = lane; q < EDIT_WIN; q += 64u) {
      const int p = lo + (int)q;
      uint8_t ca = nts::CODE_INVALID, cb = nts::CODE_INVALID;
      if (p >= 0 && p < dx) {
        ca = pa[p];
        bad |= ca >= nts::CODE_INVALID;
      }
      if (p >= 0 && p < dy) {
        cb = flip ? pb[-(int64_t)p] : pb[p];
        bad |= cb >= nts::CODE_INVALID;
        if (flip && cb < nts::CODE_INVALID) cb = (uint8_t)(3u - cb); // (the complement the canonical hash uses: A <-> T, C <-> G)
      }
      s_a[wv][q] = ca;
      s_b[wv][q] = cb;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // (one wave writes and reads its own rows: LDS serves a wave in order)
    if (__any(bad)) break;                                 // (the same for every lane of the wave)
    const int t1 = T < t0 + (int)EDIT_CHUNK - 1 ? T : t0 + (int)EDIT_CHUNK - 1;
    for (int t = t0; t <= t1; ++t) {
      uint32_t left = __shfl_up(val, 1u), right = __shfl_down(val, 1u);
      if (lane == 0u) left = EDIT_INF;
      if (lane == 63u) right = EDIT_INF;
      const int i2 = t - d, j2 = t + d;
      if (in_band && !(i2 & 1) && i2 >= 0 && j2 >= 0 && (i2 >> 1) <= dx && (j2 >> 1) <= dy) {
        const int ia = (i2 >> 1) - 1 - lo, ib = (j2 >> 1) - 1 - lo; // (row or column 0: a slot outside the string, and val is EDIT_INF)
        uint32_t best = val + (s_a[wv][ia] != s_b[wv][ib] ? 1u : 0u);
        best = best < left + 1u ? best : left + 1u;
        best = best < right + 1u ? best : right + 1u;
        val = best < EDIT_INF ? best : EDIT_INF;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
  const bool any_bad = __any(bad);
  const uint32_t D = __shfl(val, (int)W + delta); // (|delta| <= W was checked: a lane of the band)
  if (lane == 0) dist[sidx] = any_bad ? NTS_EDIT_INVALID : ((D + (uint32_t)ad) >> 1) > W ? NTS_EDIT_OVERBAND : D;
}

// what segment i brings to its interval's sums
__global__ __launch_bounds__(256) void k_edit_kinds(const nts_iv_segment* __restrict__ segs, const uint32_t* __restrict__ dist, uint64_t n,
                                                    nts_iv_identity* __restrict__ agg)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const nts_iv_segment s = segs[i];
  const uint32_t D = dist[i];
  nts_iv_identity a{ 0, 0, 0, 1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };
  if (s.kind == NTS_SEG_BACKWARD) a.backward = 1u;
  if (s.kind == NTS_SEG_LONG) a.too_long = 1u;
  if (s.kind == NTS_SEG_OFFBAND) a.offband = 1u;
  if (D == NTS_EDIT_INVALID) a.invalid = 1u;
  if (D == NTS_EDIT_OVERBAND) a.overband = 1u;
  if (D < NTS_EDIT_INVALID) {
    a.aligned = 1u;
    a.aligned_a = s.dx;
    a.aligned_b = (uint32_t)s.dy;
    a.edits = D;
  }
  agg[i] = a;
}

__global__ __launch_bounds__(256) void k_edit_store(const uint32_t* __restrict__ iv, const nts_iv_identity* __restrict__ agg,
                                                    const uint64_t* __restrict__ n_keys, uint64_t cap, uint64_t n_iv, nts_iv_identity* __restrict__ out)
{
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cap || j >= *n_keys) return;
  const uint32_t i = iv[j];
  if (i < n_iv) out[i] = agg[j];
}

// the clipped start and length of an interval, as the sampling calls clip
int edit_clip(nts_ctx* ctx, const nts_genome* g, const nts_interval& iv, uint64_t* at, uint32_t* len)
{
  if (iv.rec >= g->n_rec) return fail(ctx, NTS_EINVAL, "nts_edit_segments: record index out of range");
  const uint64_t rl = g->rec_len[iv.rec], a = std::min(iv.start, rl), b = std::min(iv.end, rl);
  if (b > a && b - a > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_edit_segments: an interval of 2^32 bases or more");
  *at = g->rec_off[iv.rec] + a;
  *len = b > a ? (uint32_t)(b - a) : 0u;
  return NTS_OK;
}

// the host checks on segments, intervals and flip that nts_edit_segments and nts_edit_script share, and what the kernels need of
// every interval that has a segment
int edit_prepare(nts_ctx* ctx, const nts_genome* ga, const nts_genome* gb, const nts_interval* iv_a, const nts_interval* iv_b,
                 const nts_iv_segment* segs, uint64_t n, uint64_t n_iv, const uint8_t* flip, uint32_t band, std::vector<EditIv>& ivs)
{
  if (n > 0xFFFFFFFFull || n_iv > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_edit_segments: 2^32 segments or intervals or more");
  ivs.resize(n_iv);
  std::vector<uint8_t> used(n_iv, 0);
  for (uint64_t i = 0; i < n; ++i) {
    if (segs[i].iv_a >= n_iv) return fail(ctx, NTS_EINVAL, "nts_edit_segments: a segment names an interval at or beyond n_iv_a");
    if (i && segs[i].iv_a < segs[i - 1].iv_a) return fail(ctx, NTS_EINVAL, "nts_edit_segments: the segments are not in iv_a order");
    used[segs[i].iv_a] = 1;
  }
  for (uint64_t i = 0; i < n_iv; ++i) {
    ivs[i] = { 0, 0, 0, 0, 0, 0 };
    if (!used[i]) continue; // (an interval without a segment may have no mate: its iv_b entry is not read)
    if (flip[i] > 1) return fail(ctx, NTS_EINVAL, "nts_edit_segments: flip is 0 or 1");
    ivs[i].flip = flip[i];
    if (int rc = edit_clip(ctx, ga, iv_a[i], &ivs[i].a0, &ivs[i].la)) return rc;
    if (int rc = edit_clip(ctx, gb, iv_b[i], &ivs[i].b0, &ivs[i].lb)) return rc;
  }
  for (uint64_t i = 0; i < n; ++i) {
    const nts_iv_segment& s = segs[i];
    if (s.kind != NTS_SEG_CANDIDATE) continue;
    const EditIv& v = ivs[s.iv_a];
    const int64_t delta = (int64_t)s.dy - (int64_t)s.dx;
    if (s.dx < 1 || s.dy < 1 || s.dx > EDIT_MAX_LEN || s.dy > (int32_t)EDIT_MAX_LEN || delta > (int64_t)band || -delta > (int64_t)band ||
        (uint64_t)s.x + s.dx > v.la || (uint64_t)s.y_lo + (uint32_t)s.dy > v.lb)
      return fail(ctx, NTS_EINVAL, "nts_edit_segments: a candidate segment leaves its interval, the band or the length limit");
  }
  return NTS_OK;
}

// the sums per interval of what `kinds` makes of every segment: one reduction by key over iv_a (segments arrive in iv_a order), stored at
// out[iv_a].  nts_edit_segments and nts_edit_wide (csrc/nts_edit_wide.inc) differ in the kinds kernel alone.
using EditKinds = void (*)(const nts_iv_segment*, const uint32_t*, uint64_t, nts_iv_identity*);

hipError_t edit_sums(nts_ctx* ctx, EditKinds kinds, const nts_iv_segment* d_seg, const uint32_t* d_dist, uint64_t n, uint64_t n_iv, nts_iv_identity* d_agg,
                     nts_iv_identity* d_uagg, uint32_t* d_uiv, uint64_t* d_num, nts_iv_identity* d_out)
{
  ScopedTimer t(ctx, "edit_reduce");
  NTS_LAUNCH(kinds, IVL_GRID(n), d_seg, d_dist, n, d_agg);
  auto keys = rocprim::make_transform_iterator(d_seg, EditIvOf());
  size_t tmp = 0;
  hipError_t e = rocprim::reduce_by_key(nullptr, tmp, keys, d_agg, n, d_uiv, d_uagg, d_num, EditAdd(), rocprim::equal_to<uint32_t>(), ctx->stream);
  void* d_tmp = e == hipSuccess ? ws_get(ctx, "ivs_tmp", std::max<size_t>(tmp, 16)) : nullptr;
  if (e == hipSuccess && !d_tmp) e = hipErrorOutOfMemory;
  if (e == hipSuccess) e = rocprim::reduce_by_key(d_tmp, tmp, keys, d_agg, n, d_uiv, d_uagg, d_num, EditAdd(), rocprim::equal_to<uint32_t>(), ctx->stream);
  if (e == hipSuccess) NTS_LAUNCH(k_edit_store, IVL_GRID(n), (const uint32_t*)d_uiv, (const nts_iv_identity*)d_uagg, (const uint64_t*)d_num, n, n_iv, d_out);
  return e;
}

int edit_segments_run(nts_ctx* ctx, const nts_genome* ga, const nts_genome* gb, const nts_interval* iv_a, const nts_interval* iv_b,
                      const nts_iv_segment* segs, uint64_t n, uint64_t n_iv, const uint8_t* flip, uint32_t band, nts_iv_identity* per_iv,
                      uint32_t* dist_out)
{
  std::vector<EditIv> ivs;
  if (int rc = edit_prepare(ctx, ga, gb, iv_a, iv_b, segs, n, n_iv, flip, band, ivs)) return rc;
  if (n_iv) memset(per_iv, 0, n_iv * sizeof(nts_iv_identity));
  if (n == 0 || n_iv == 0) return NTS_OK;
  NTS_WS(d_ivs, EditIv*, "edit_ivs", n_iv * sizeof(EditIv));
  NTS_WS(d_seg, nts_iv_segment*, "edit_seg", n * sizeof(nts_iv_segment));
  NTS_WS(d_dist, uint32_t*, "edit_dist", n * 4);
  NTS_WS(d_agg, nts_iv_identity*, "edit_agg", n * sizeof(nts_iv_identity));
  NTS_WS(d_uagg, nts_iv_identity*, "edit_uagg", n * sizeof(nts_iv_identity));
  NTS_WS(d_uiv, uint32_t*, "edit_uiv", n * 4);
  NTS_WS(d_num, uint64_t*, "edit_num", 8);
  NTS_WS(d_out, nts_iv_identity*, "edit_out", n_iv * sizeof(nts_iv_identity));
  hipError_t e = hipMemcpyAsync(d_ivs, ivs.data(), n_iv * sizeof(EditIv), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_seg, segs, n * sizeof(nts_iv_segment), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_out, 0, n_iv * sizeof(nts_iv_identity), ctx->stream);
  if (e != hipSuccess) hipStreamSynchronize(ctx->stream); // (before `ivs` goes away)
  HIP_TRY(ctx, e);
  {
    ScopedTimer t(ctx, "edit_segments", true);
    NTS_LAUNCH(k_edit_wave, dim3((uint32_t)((n + EDIT_WAVES - 1) / EDIT_WAVES)), dim3(EDIT_WAVES * 64), 0, ctx->stream, (const uint8_t*)ga->d_code + PAD,
               (const uint8_t*)gb->d_code + PAD, (const EditIv*)d_ivs, n_iv, (const nts_iv_segment*)d_seg, n, band, d_dist);
  }
  hipError_t e_reduce = edit_sums(ctx, k_edit_kinds, d_seg, d_dist, n, n_iv, d_agg, d_uagg, d_uiv, d_num, d_out);
  if (e_reduce == hipSuccess) e_reduce = hipGetLastError();
  if (e_reduce == hipSuccess) e_reduce = hipMemcpyAsync(per_iv, d_out, n_iv * sizeof(nts_iv_identity), hipMemcpyDeviceToHost, ctx->stream);
  if (e_reduce == hipSuccess && dist_out) e_reduce = hipMemcpyAsync(dist_out, d_dist, n * 4, hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t e_sync = hipStreamSynchronize(ctx->stream); // (whatever happened: `ivs` was the source of an asynchronous copy)
  HIP_TRY(ctx, e_reduce);
  HIP_TRY(ctx, e_sync);
  return NTS_OK;
}

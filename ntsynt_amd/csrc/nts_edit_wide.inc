// ---- the exact edit distance of the stretches the 31-diagonal band leaves out, up to E edits (nts_edit_wide; ntsynt_amd/assess.py ----
// block_identity with max_edits > 0).  docs/design/04_18_block_identity_wide.md.  Input: the segments, intervals and flips of
// nts_edit_segments and its dist_out.  The work set: kind offband with |dy - dx| <= E, and candidates the narrow pass called overband.
// Plan (rocprim): a selection over a counting iterator keeps the work set's indices.
// k_edit_wide: one 64-lane wave per work-set segment, WIDE_WAVES waves per workgroup.  The furthest-reaching recurrence over ALL
// diagonals d = j - i (i bases of A against j bases of B): F_e[d] = the furthest row i on diagonal d that at most e edits reach, D = the
// least e with F_e[delta] = n.  Rows e - 1 and e are live, in LDS as int32: two rows of 2 E + 3 entries per wave (index d + E + 1; WIDE_NONE
// where nothing was written).  Row e: the lanes stride over d in [max(-e, -n, delta - (E - e)), min(e, m, delta + (E - e))] in steps of 64
// -- a diagonal further than E - e from delta cannot reach it within the edits that remain --, each entry takes the largest in-matrix
// value of F_{e-1}[d] (stay), F_{e-1}[d] + 1 (SUB), F_{e-1}[d+1] + 1 (DEL) and F_{e-1}[d-1] (INS) as k_edit_script does, then slides along
// equal bases: byte loads from the two genomes, only inside the two strings.  The loop over e ends at the first e with F_e[delta] = n, or
// behind e = E (overband).  Before it the wave reads every base of both strings once: a code >= CODE_INVALID makes the segment `invalid`
// (the recurrence alone skips the bases of an indel).  No atomic, no launch per segment, no floating point.

constexpr uint32_t WIDE_WAVES = 2; // 2 waves x 2 rows x (2 E + 3) x 4 B: 32 784 B per workgroup at E = 1023, four workgroups of a CU's 160 KiB
constexpr uint32_t WIDE_MAX_EDITS = 1023;
constexpr int32_t WIDE_NONE = -1;

// segment i belongs to the work set (host and device: the host counts with it what the selection keeps)
struct WideKeep
{
  const nts_iv_segment* segs;
  const uint32_t* dist;
  uint32_t max_edits;
  __host__ __device__ bool operator()(uint32_t i) const
  {
    const uint32_t d = dist[i];
    if (d == NTS_EDIT_OVERBAND) return true;
    if (d != NTS_EDIT_PASSED || segs[i].kind != NTS_SEG_OFFBAND) return false;
    const int64_t delta = (int64_t)segs[i].dy - (int64_t)segs[i].dx;
    return (delta < 0 ? -delta : delta) <= (int64_t)max_edits;
  }
};

__global__ __launch_bounds__(WIDE_WAVES * 64) void k_edit_wide(const uint8_t* __restrict__ code_a, const uint8_t* __restrict__ code_b,
                                                               const EditIv* __restrict__ ivs, uint64_t n_iv, const nts_iv_segment* __restrict__ segs,
                                                               uint64_t n_segs, uint32_t E, const uint32_t* __restrict__ work,
                                                               const uint64_t* __restrict__ n_work, uint64_t cap_work, uint32_t* __restrict__ dist)
{
  extern __shared__ int32_t s_wide[]; // WIDE_WAVES x 2 rows x (2 E + 3)
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t w = (uint64_t)blockIdx.x * WIDE_WAVES + wv;
  if (w >= cap_work || w >= *n_work) return;
  const uint32_t sidx = work[w];
  // (the host refused all of what follows before the launch: a lane still touches nothing outside its strings and its rows)
  if (sidx >= n_segs || E < 3u || E > WIDE_MAX_EDITS) return;
  const nts_iv_segment s = segs[sidx];
  const int n = (int)s.dx, m = s.dy;
  const int delta = m - n, ad = delta < 0 ? -delta : delta;
  EditIv v{ 0, 0, 0, 0, 0, 0 };
  if (s.iv_a < n_iv) v = ivs[s.iv_a];
  if ((s.kind != NTS_SEG_CANDIDATE && s.kind != NTS_SEG_OFFBAND) || n < 1 || m < 1 || n > (int)EDIT_MAX_LEN || m > (int)EDIT_MAX_LEN || ad > (int)E ||
      (uint64_t)s.x + (uint32_t)n > v.la || (uint64_t)s.y_lo + (uint32_t)m > v.lb)
    return;
  const uint8_t* const pa = code_a + v.a0 + s.x;
  const bool flip = v.flip != 0;
  const uint8_t* const pb = flip ? code_b + v.b0 + (v.lb - 1u - s.y_lo) : code_b + v.b0 + s.y_lo; // (as k_edit_wave reads B)

  // every base of both strings once: what is not A, C, G or T makes the segment invalid, wherever an alignment would pass it
  bool bad = false;
  for (int p = (int)lane; p < n; p += 64) bad |= pa[p] >= nts::CODE_INVALID;
  for (int q = (int)lane; q < m; q += 64) bad |= (flip ? pb[-(int64_t)q] : pb[q]) >= nts::CODE_INVALID;
  if (__any(bad)) {
    if (lane == 0) dist[sidx] = NTS_EDIT_INVALID;
    return;
  }

  const int iE = (int)E, stride = 2 * iE + 3, off = iE + 1; // entry d of a row at index d + off: -E - 1 .. E + 1
  int32_t* const rows = s_wide + (size_t)wv * 2u * (uint32_t)stride;
  for (int q = (int)lane; q < 2 * stride; q += 64) rows[q] = WIDE_NONE;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // (one wave writes and reads its own rows: LDS serves a wave in order)

  uint32_t result = NTS_EDIT_OVERBAND;
  for (int e = 0; e <= iE; ++e) {
    int32_t* const cur = rows + (e & 1) * stride;
    const int32_t* const prev = rows + ((e & 1) ^ 1) * stride;
    // the row's diagonals: inside the matrix, within e of the main one, within the E - e edits that remain of delta
    int dlo = -e > -n ? -e : -n, dhi = e < m ? e : m;
    if (delta - (iE - e) > dlo) dlo = delta - (iE - e);
    if (delta + (iE - e) < dhi) dhi = delta + (iE - e);
    bool found = false;
    for (int base = dlo; base <= dhi; base += 64) { // (the same trips for every lane)
      const int d = base + (int)lane;
      if (d <= dhi) {
        const int lo = d < 0 ? -d : 0, hi = n < m - d ? n : m - d; // the rows of diagonal d inside the matrix: lo <= hi for -n <= d <= m
        int32_t cand = WIDE_NONE;
        if (e == 0) {
          cand = 0; // (dlo = dhi = 0)
        } else {
          const int32_t stay = prev[d + off], right = prev[d + 1 + off], left = prev[d - 1 + off]; // (indices 0 .. 2 E + 2)
          if (stay >= 0) cand = stay + 1 <= hi ? stay + 1 : stay;
          if (right >= 0 && right + 1 >= lo && right + 1 <= hi && right + 1 > cand) cand = right + 1;
          if (left >= lo && left <= hi && left > cand) cand = left;
        }
        if (cand >= 0) {
          while (cand < hi) { // (cand >= lo: cand + d >= 0; cand < hi: both positions inside the strings)
            const uint8_t ca = pa[cand], cb = flip ? (uint8_t)(3u - pb[-(int64_t)(cand + d)]) : pb[cand + d];
            if (ca != cb) break;
            ++cand;
          }
        }
        cur[d + off] = cand;
        found |= d == delta && cand == n;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (__any(found)) {
      result = (uint32_t)e;
      break;
    }
  }
  if (lane == 0) dist[sidx] = result;
}

// what segment i brings to its interval's sums after the wide pass: k_edit_kinds, but an offband segment counts as offband only while
// it is still passed (one the wide pass aligned, or called invalid or overband, counts as that)
__global__ __launch_bounds__(256) void k_edit_wide_kinds(const nts_iv_segment* __restrict__ segs, const uint32_t* __restrict__ dist, uint64_t n,
                                                         nts_iv_identity* __restrict__ agg)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const nts_iv_segment s = segs[i];
  const uint32_t D = dist[i];
  nts_iv_identity a{ 0, 0, 0, 1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };
  if (s.kind == NTS_SEG_BACKWARD) a.backward = 1u;
  if (s.kind == NTS_SEG_LONG) a.too_long = 1u;
  if (s.kind == NTS_SEG_OFFBAND && D == NTS_EDIT_PASSED) a.offband = 1u;
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

int edit_wide_run(nts_ctx* ctx, const nts_genome* ga, const nts_genome* gb, const nts_interval* iv_a, const nts_interval* iv_b,
                  const nts_iv_segment* segs, uint64_t n, uint64_t n_iv, const uint8_t* flip, uint32_t band, uint32_t max_edits, const uint32_t* dist,
                  nts_iv_identity* per_iv, uint32_t* dist_out)
{
  std::vector<EditIv> ivs;
  if (int rc = edit_prepare(ctx, ga, gb, iv_a, iv_b, segs, n, n_iv, flip, band, ivs)) return rc;
  // dist is what nts_edit_segments gives a segment of this kind; the offband segments of the work set lie inside their intervals
  const WideKeep keep{ segs, dist, max_edits };
  uint64_t n_work = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const nts_iv_segment& s = segs[i];
    const uint32_t d = dist[i];
    const int64_t delta = (int64_t)s.dy - (int64_t)s.dx, ad = delta < 0 ? -delta : delta;
    bool fits;
    if (s.kind == NTS_SEG_CANDIDATE)
      fits = d == NTS_EDIT_INVALID || d == NTS_EDIT_OVERBAND || (d < NTS_EDIT_INVALID && (uint64_t)d + (uint64_t)ad <= 2ull * band + 1ull);
    else
      fits = d == (s.kind <= NTS_SEG_OFFBAND ? NTS_EDIT_PASSED : NTS_EDIT_NOT_CANDIDATE);
    if (!fits) return fail(ctx, NTS_EINVAL, "nts_edit_wide: dist of segment " + std::to_string(i) + " is not what nts_edit_segments gives its kind");
    if (!keep((uint32_t)i)) continue;
    ++n_work;
    if (s.kind != NTS_SEG_OFFBAND) continue; // (a candidate: edit_prepare checked it)
    const EditIv& v = ivs[s.iv_a];
    if (s.dx < 1 || s.dy < 1 || s.dx > EDIT_MAX_LEN || s.dy > (int32_t)EDIT_MAX_LEN || (uint64_t)s.x + s.dx > v.la || (uint64_t)s.y_lo + (uint32_t)s.dy > v.lb)
      return fail(ctx, NTS_EINVAL, "nts_edit_wide: an offband segment of the work set leaves its interval or the length limit");
  }
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
  NTS_WS(d_work, uint32_t*, "edit_work", n * 4);
  NTS_WS(d_nwork, uint64_t*, "edit_nwork", 8);
  hipError_t e = hipMemcpyAsync(d_ivs, ivs.data(), n_iv * sizeof(EditIv), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_seg, segs, n * sizeof(nts_iv_segment), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_dist, dist, n * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_out, 0, n_iv * sizeof(nts_iv_identity), ctx->stream);
  if (e != hipSuccess) hipStreamSynchronize(ctx->stream); // (before `ivs` goes away)
  HIP_TRY(ctx, e);
  hipError_t e_run = hipSuccess;
  if (n_work) {
    {
      ScopedTimer t(ctx, "edit_wide_plan");
      auto flags = rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0), WideKeep{ d_seg, d_dist, max_edits });
      size_t tmp = 0;
      e_run = rocprim::select(nullptr, tmp, rocprim::counting_iterator<uint32_t>(0), flags, d_work, d_nwork, n, ctx->stream);
      void* d_tmp = e_run == hipSuccess ? ws_get(ctx, "ivs_tmp", std::max<size_t>(tmp, 16)) : nullptr;
      if (e_run == hipSuccess && !d_tmp) e_run = hipErrorOutOfMemory;
      if (e_run == hipSuccess) e_run = rocprim::select(d_tmp, tmp, rocprim::counting_iterator<uint32_t>(0), flags, d_work, d_nwork, n, ctx->stream);
    }
    if (e_run == hipSuccess) {
      ScopedTimer t(ctx, "edit_wide", true);
      const size_t lds = (size_t)WIDE_WAVES * 2u * (2u * max_edits + 3u) * sizeof(int32_t);
      NTS_LAUNCH(k_edit_wide, dim3((uint32_t)((n_work + WIDE_WAVES - 1) / WIDE_WAVES)), dim3(WIDE_WAVES * 64), lds, ctx->stream,
                 (const uint8_t*)ga->d_code + PAD, (const uint8_t*)gb->d_code + PAD, (const EditIv*)d_ivs, n_iv, (const nts_iv_segment*)d_seg, n, max_edits,
                 (const uint32_t*)d_work, (const uint64_t*)d_nwork, n_work, d_dist);
    }
  }
  if (e_run == hipSuccess)
    e_run = edit_sums(ctx, k_edit_wide_kinds, d_seg, d_dist, n, n_iv, d_agg, d_uagg, d_uiv, d_num, d_out);
  if (e_run == hipSuccess) e_run = hipGetLastError();
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(per_iv, d_out, n_iv * sizeof(nts_iv_identity), hipMemcpyDeviceToHost, ctx->stream);
  if (e_run == hipSuccess && dist_out) e_run = hipMemcpyAsync(dist_out, d_dist, n * 4, hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t e_sync = hipStreamSynchronize(ctx->stream); // (whatever happened: `ivs` was the source of an asynchronous copy)
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  return NTS_OK;
}

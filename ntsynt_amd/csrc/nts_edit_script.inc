// ---- the edit script behind every aligned segment's distance (nts_edit_script; ntsynt_amd/assess.py block_variants). ----
// docs/design/04_17_block_variants.md.  Input: the segments, intervals and flips of nts_edit_segments and its dist_out.  Output: for
// every segment with a distance D >= 1 the D edits of the canonical script, in path order, at first[seg] .. first[seg] + D - 1.
// Plan (rocprim): an exclusive scan of D (0 where dist is no distance) gives `first`; a selection keeps the segments with D >= 1.
// k_edit_script: one 64-lane wave per kept segment, SCRIPT_WAVES waves per workgroup, lane l on diagonal d = l - W (d = j - i).  Row e
// of F (e = 0 .. D <= 63, 64 int32 entries, lane 63 and every lane outside the band hold SCRIPT_NONE) lives in LDS: F[e][d] = the
// furthest row i on diagonal d that at most e edits reach inside the band.  Forward: F[0][0] = the common prefix; row e takes, per
// lane, the largest of F[e-1][d] (stay), F[e-1][d] + 1 (SUB), F[e-1][d+1] + 1 (DEL) and F[e-1][d-1] (INS) that lies in the diagonal's
// range of the matrix, then slides along equal bases -- byte loads from the two genomes, only inside the two strings.  The wave goes
// on only if F[D][delta] = n and F[D-1][delta] < n: then D is the distance (every path of D - 1 edits stays inside the band).
// Traceback from (n, m): the 64 lanes compare the 64 positions back along the diagonal, a ballot gives the match run (rule 1); at the
// mismatch T[i-1][j-1] = e - 1 exactly when F[e-1][d] >= i - 1 (SUB) and T[i-1][j] = e - 1 exactly when F[e-1][d+1] >= i - 1 (DEL),
// otherwise INS; the op goes to slot first[seg] + e - 1.  No atomic, no launch per segment, no floating point.

constexpr int32_t SCRIPT_NONE = -1;
constexpr uint32_t SCRIPT_WAVES = 2;  // 2 waves x 64 rows x 64 lanes x 4 B = 32 KiB per workgroup: five workgroups, ten waves per CU
constexpr uint32_t SCRIPT_ROWS = 64;  // e = 0 .. 2 W + 1 at W = 31
static_assert(2 * EDIT_MAX_BAND + 1 < SCRIPT_ROWS, "a row per edit count up to the largest accepted distance");
static_assert(SCRIPT_WAVES * SCRIPT_ROWS * 64 * 4 <= 64 * 1024, "static LDS of one workgroup");
static_assert(sizeof(nts_edit_op) == 16, "the C ABI's layout");

struct ScriptCount // what a segment's dist adds to the number of ops
{
  __host__ __device__ uint64_t operator()(uint32_t d) const { return d < NTS_EDIT_INVALID ? d : 0u; }
};

struct ScriptKeep
{
  __host__ __device__ bool operator()(uint32_t d) const { return d >= 1u && d < NTS_EDIT_INVALID; }
};

// the codes of A[p] and of the oriented B[q]; what is not A, C, G or T equals nothing, itself included
__device__ __forceinline__ uint32_t script_a(const uint8_t* pa, int p, bool& bad)
{
  const uint8_t c = pa[p];
  if (c >= nts::CODE_INVALID) {
    bad = true;
    return 0x100u;
  }
  return c;
}

__device__ __forceinline__ uint32_t script_b(const uint8_t* pb, int q, bool flip, bool& bad)
{
  const uint8_t c = flip ? pb[-(int64_t)q] : pb[q];
  if (c >= nts::CODE_INVALID) {
    bad = true;
    return 0x200u;
  }
  return flip ? 3u - c : c;
}

__global__ __launch_bounds__(SCRIPT_WAVES * 64) void k_edit_script(const uint8_t* __restrict__ code_a, const uint8_t* __restrict__ code_b,
                                                                   const EditIv* __restrict__ ivs, uint64_t n_iv, const nts_iv_segment* __restrict__ segs,
                                                                   uint64_t n_segs, uint32_t W, const uint32_t* __restrict__ dist,
                                                                   const uint64_t* __restrict__ first, const uint32_t* __restrict__ kept,
                                                                   const uint64_t* __restrict__ n_kept, uint64_t cap_kept, nts_edit_op* __restrict__ ops,
                                                                   uint64_t n_ops, uint32_t* __restrict__ status)
{
  __shared__ int32_t s_f[SCRIPT_WAVES][SCRIPT_ROWS][64];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t w = (uint64_t)blockIdx.x * SCRIPT_WAVES + wv;
  if (w >= cap_kept) return;
  if (w >= *n_kept) {
    if (lane == 0) status[w] = SCRIPT_OK;
    return;
  }
  const uint32_t sidx = kept[w];
  // (the host refused all of what follows before the launch: a lane still touches nothing outside its strings, its rows and its slots)
  if (sidx >= n_segs) {
    if (lane == 0) status[w] = 0u;
    return;
  }
  const nts_iv_segment s = segs[sidx];
  const uint32_t D = dist[sidx];
  const uint64_t slot0 = first[sidx];
  const int n = (int)s.dx, m = s.dy;
  const int delta = m - n, ad = delta < 0 ? -delta : delta;
  EditIv v{ 0, 0, 0, 0, 0, 0 };
  if (s.iv_a < n_iv) v = ivs[s.iv_a];
  if (s.kind != NTS_SEG_CANDIDATE || W < 1 || W > EDIT_MAX_BAND || n < 1 || m < 1 || n > (int)EDIT_MAX_LEN || m > (int)EDIT_MAX_LEN || ad > (int)W ||
      (uint64_t)s.x + (uint32_t)n > v.la || (uint64_t)s.y_lo + (uint32_t)m > v.lb || D < 1 || D >= SCRIPT_ROWS || D + (uint32_t)ad > 2u * W + 1u ||
      slot0 > n_ops || D > n_ops - slot0) {
    if (lane == 0) status[w] = sidx;
    return;
  }
  const uint8_t* const pa = code_a + v.a0 + s.x;
  const bool flip = v.flip != 0;
  const uint8_t* const pb = flip ? code_b + v.b0 + (v.lb - 1u - s.y_lo) : code_b + v.b0 + s.y_lo; // (as k_edit_wave reads B)
  const int d = (int)lane - (int)W;
  const bool in_band = lane <= 2u * W;
  const int lo = d < 0 ? -d : 0, hi = n < m - d ? n : m - d; // the rows of diagonal d inside the matrix (none where hi < lo)
  int32_t(*F)[64] = s_f[wv];
  bool bad = false;

  // forward
  int32_t cur = SCRIPT_NONE;
  for (uint32_t e = 0; e <= D; ++e) {
    int32_t cand = SCRIPT_NONE;
    if (e == 0) {
      if (lane == W) cand = 0;
    } else if (in_band) {
      const int32_t left = lane > 0u ? F[e - 1][lane - 1u] : SCRIPT_NONE, right = F[e - 1][lane + 1u]; // (lane + 1 <= 63: SCRIPT_NONE beyond the band)
      if (cur >= 0) cand = cur + 1 <= hi ? cur + 1 : cur;
      if (right >= 0 && right + 1 >= lo && right + 1 <= hi && right + 1 > cand) cand = right + 1;
      if (left >= lo && left <= hi && left > cand) cand = left;
    }
    if (cand >= 0) {
      while (cand < hi) { // (cand >= lo >= 0 and cand + d >= 0; cand < hi: both positions inside the strings)
        if (script_a(pa, cand, bad) != script_b(pb, cand + d, flip, bad)) break;
        ++cand;
      }
    }
    cur = cand;
    F[e][lane] = cur;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // (one wave writes and reads its own rows: LDS serves a wave in order)
  }
  // consistency: D edits reach the corner, D - 1 do not; no base met that is not A, C, G or T
  const int32_t end_d = F[D][(int)W + delta], end_less = F[D - 1][(int)W + delta];
  if (__any(bad) || end_d != n || end_less >= n) {
    if (lane == 0) status[w] = sidx;
    return;
  }

  // traceback, the whole wave at one cell (i, j) of value e
  int i = n, j = m;
  uint32_t e = D;
  bool broken = false;
  while (i > 0 || j > 0) {
    nts_edit_op op{ sidx, 0u, 0u, 0u, 0xFFu, 0xFFu, 0u };
    if (i > 0 && j > 0) {
      const int k = (int)lane;
      bool eq = false, bad_here = false;
      if (i - 1 - k >= 0 && j - 1 - k >= 0) eq = script_a(pa, i - 1 - k, bad_here) == script_b(pb, j - 1 - k, flip, bad_here);
      const uint64_t differ = ~__ballot(eq);
      const int run = differ ? __builtin_ctzll(differ) : 64;
      i -= run;
      j -= run;
      if (run == 64 || i == 0 || j == 0) continue;
      if (__any(bad_here && k == run)) broken = true; // (the mismatch is a base the forward pass did not meet: dist was not this segment's)
      if (e == 0 || broken) {
        broken = true;
        break;
      }
      const int ld = (int)W + (j - i); // the lane of the cell's diagonal: inside the band, as every cell of an optimal path is
      if (ld < 0 || ld > 2 * (int)W) {
        broken = true;
        break;
      }
      if (F[e - 1][ld] >= i - 1) {
        op.op = NTS_OP_SUB, op.p = (uint32_t)(i - 1), op.q = (uint32_t)(j - 1);
        --i, --j;
      } else if (F[e - 1][ld + 1] >= i - 1) {
        op.op = NTS_OP_DEL, op.p = (uint32_t)(i - 1), op.q = (uint32_t)j;
        --i;
      } else {
        op.op = NTS_OP_INS, op.p = (uint32_t)i, op.q = (uint32_t)(j - 1);
        --j;
      }
    } else if (i > 0) { // column 0: only DEL
      op.op = NTS_OP_DEL, op.p = (uint32_t)(i - 1), op.q = 0u;
      --i;
    } else { // row 0: only INS
      op.op = NTS_OP_INS, op.p = 0u, op.q = (uint32_t)(j - 1);
      --j;
    }
    if (e == 0) {
      broken = true;
      break;
    }
    if (lane == 0) {
      bool unused = false;
      if (op.op != NTS_OP_INS) op.base_a = (uint8_t)script_a(pa, (int)op.p, unused);
      if (op.op != NTS_OP_DEL) op.base_b = (uint8_t)script_b(pb, (int)op.q, flip, unused);
      ops[slot0 + e - 1u] = op; // (1 <= e <= D: a slot of this segment)
    }
    --e;
  }
  if (lane == 0) status[w] = (broken || e != 0u) ? sidx : SCRIPT_OK;
}

int edit_script_run(nts_ctx* ctx, const nts_genome* ga, const nts_genome* gb, const nts_interval* iv_a, const nts_interval* iv_b,
                    const nts_iv_segment* segs, uint64_t n, uint64_t n_iv, const uint8_t* flip, uint32_t band, const uint32_t* dist, nts_edit_op** ops,
                    uint64_t* n_ops, uint64_t* first)
{
  *ops = nullptr;
  *n_ops = 0;
  std::vector<EditIv> ivs;
  if (int rc = edit_prepare(ctx, ga, gb, iv_a, iv_b, segs, n, n_iv, flip, band, ivs)) return rc;
  uint64_t total = 0, kept = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (dist[i] >= NTS_EDIT_INVALID) continue;
    if (segs[i].kind != NTS_SEG_CANDIDATE) return fail(ctx, NTS_EINVAL, "nts_edit_script: a distance on segment " + std::to_string(i) + ", which is no candidate");
    const int64_t delta = (int64_t)segs[i].dy - (int64_t)segs[i].dx;
    // (D + |dy - dx|) / 2 <= band, as nts_edit_segments accepts a distance
    if ((uint64_t)dist[i] + (uint64_t)(delta < 0 ? -delta : delta) > 2ull * band + 1ull)
      return fail(ctx, NTS_EINVAL, "nts_edit_script: the distance of segment " + std::to_string(i) + " lies beyond the band");
    total += dist[i];
    kept += dist[i] >= 1u;
  }
  if (total > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_edit_script: 2^32 edits or more");
  if (first) first[n] = total;
  if (n == 0) return NTS_OK;
  NTS_WS(d_ivs, EditIv*, "edit_ivs", std::max<size_t>(n_iv, 1) * sizeof(EditIv));
  NTS_WS(d_seg, nts_iv_segment*, "edit_seg", n * sizeof(nts_iv_segment));
  NTS_WS(d_dist, uint32_t*, "edit_dist", n * 4);
  NTS_WS(d_first, uint64_t*, "edit_first", n * 8);
  NTS_WS(d_kept, uint32_t*, "edit_kept", n * 4);
  NTS_WS(d_status, uint32_t*, "edit_status", std::max<uint64_t>(kept, 1) * 4);
  NTS_WS(d_num, uint64_t*, "edit_num", 8);
  NTS_WS(d_worst, uint32_t*, "edit_worst", 4);
  NTS_WS(d_ops, nts_edit_op*, "edit_ops", std::max<uint64_t>(total, 1) * sizeof(nts_edit_op));
  hipError_t e = hipMemcpyAsync(d_ivs, ivs.data(), n_iv * sizeof(EditIv), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_seg, segs, n * sizeof(nts_iv_segment), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_dist, dist, n * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) hipStreamSynchronize(ctx->stream); // (before `ivs` goes away)
  HIP_TRY(ctx, e);
  const hipError_t e_plan = script_plan(ctx, "edit_script_plan", rocprim::make_transform_iterator((const uint32_t*)d_dist, ScriptCount()),
                                        rocprim::make_transform_iterator((const uint32_t*)d_dist, ScriptKeep()), n, d_first, d_kept, d_num);
  auto launch = [&] {
    NTS_LAUNCH(k_edit_script, dim3((uint32_t)((kept + SCRIPT_WAVES - 1) / SCRIPT_WAVES)), dim3(SCRIPT_WAVES * 64), 0, ctx->stream,
               (const uint8_t*)ga->d_code + PAD, (const uint8_t*)gb->d_code + PAD, (const EditIv*)d_ivs, n_iv, (const nts_iv_segment*)d_seg, n, band,
               (const uint32_t*)d_dist, (const uint64_t*)d_first, (const uint32_t*)d_kept, (const uint64_t*)d_num, kept, d_ops, total, d_status);
  };
  ScriptDone done; // (kept = 0: the plan ran, nothing is launched, *ops = NULL)
  if (int rc = script_finish(ctx, e_plan, "edit_script", launch, d_status, d_worst, kept, d_ops, total, d_first, first, n, done)) return rc;
  if (done.no_memory) return fail(ctx, NTS_ENOMEM, "nts_edit_script: no host memory for the ops");
  if (done.worst != SCRIPT_OK) return fail(ctx, NTS_EINVAL, "nts_edit_script: dist is not the distance of segment " + std::to_string(done.worst));
  *ops = done.ops;
  *n_ops = total;
  return NTS_OK;
}

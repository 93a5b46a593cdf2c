// ---- how far two strings stay alignable from a fixed common start: the free-end extension (nts_edit_extend; ntsynt_amd/assess.py ----
// block_ends).  docs/design/04_20_block_ends.md.  A task names two strings: n bases of a record of genome A and m bases of a record of
// genome B, each read forwards or backwards from a record position, B complemented or not; both are cut before their first base with a
// code >= CODE_INVALID (n_v, m_v).  With T the unrestricted unit-cost edit table, among the cells (i, j), i <= n_v, j <= m_v, with
// T[i][j] <= E the result is the one with the largest S = i + j - P T[i][j]; ties: the least T, then the least d = j - i.
// k_edit_extend: one 64-lane wave per task, EXTEND_WAVES waves per workgroup.  The furthest-reaching rows of k_edit_wide
// (csrc/nts_edit_wide.inc) with no target corner: F_e[d] = the furthest row i on diagonal d that at most e edits reach, row e over
// d in [max(-e, -n_v), min(e, m_v)], no pruning; rows e - 1 and e live in LDS as int32, two rows of 2 E + 3 entries per wave (index
// d + E + 1; EXTEND_NONE where nothing was written).  The largest S over the cells with T <= E is the largest 2 F_e[d] + d - P e over
// e <= E and d, and under the order (S descending, e ascending, d ascending) the winning entry's cell has T = e.  Every lane keeps the
// best entry it computed; after row e the wave stops when n_v + m_v - P (e + 1) <= its best S (no later entry can win, or tie ahead of
// it), or behind e = E.  Byte loads from the two genomes, only at positions inside the cut strings.  No atomic, no launch per task, no
// floating point.

constexpr uint32_t EXTEND_WAVES = 2; // 2 waves x 2 rows x (2 E + 3) x 4 B: 32 784 B per workgroup at E = 1023, as k_edit_wide
constexpr uint32_t EXTEND_MAX_EDITS = 1023, EXTEND_MIN_PENALTY = 3, EXTEND_MAX_PENALTY = 255, EXTEND_MAX_LEN = 65535;
constexpr int32_t EXTEND_NONE = -1;
static_assert(sizeof(nts_extend_task) == 40 && sizeof(nts_extend_result) == 20, "the C ABI's layout");

struct ExtendTask // what the kernel needs of a task: the index of either string's first base in its genome's codes
{
  uint64_t a0, b0;
  uint32_t n, m, flags, pad;
};

// the position of the first code >= CODE_INVALID among the n bases from p in steps of `step` (n when there is none): every lane the
// least over its positions, then the wave's least
__device__ __forceinline__ int extend_cut(const uint8_t* p, int64_t step, int n, uint32_t lane)
{
  int cut = n;
  for (int q = (int)lane; q < n; q += 64)
    if (p[step * q] >= nts::CODE_INVALID && q < cut) cut = q;
  for (int w = 32; w >= 1; w >>= 1) {
    const int other = __shfl_xor(cut, w);
    cut = other < cut ? other : cut;
  }
  return cut;
}

__global__ __launch_bounds__(EXTEND_WAVES * 64) void k_edit_extend(const uint8_t* __restrict__ code_a, const uint8_t* __restrict__ code_b,
                                                                   const ExtendTask* __restrict__ tasks, uint64_t n_tasks, uint32_t P, uint32_t E,
                                                                   nts_extend_result* __restrict__ out)
{
  extern __shared__ int32_t s_extend[]; // EXTEND_WAVES x 2 rows x (2 E + 3)
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t w = (uint64_t)blockIdx.x * EXTEND_WAVES + wv;
  if (w >= n_tasks) return;
  const ExtendTask t = tasks[w];
  // (the host refused all of what follows before the launch: a lane still touches nothing outside its rows)
  if (E < 1u || E > EXTEND_MAX_EDITS || P < EXTEND_MIN_PENALTY || P > EXTEND_MAX_PENALTY || t.n > EXTEND_MAX_LEN || t.m > EXTEND_MAX_LEN) return;
  const uint8_t* const pa = code_a + t.a0;
  const uint8_t* const pb = code_b + t.b0;
  const int64_t sa = (t.flags & NTS_EXTEND_A_BACKWARDS) ? -1 : 1, sb = (t.flags & NTS_EXTEND_B_BACKWARDS) ? -1 : 1;
  const bool comp = (t.flags & NTS_EXTEND_B_COMPLEMENT) != 0;

  // the cut first: the recurrence never loads at or beyond n or m
  const int n = extend_cut(pa, sa, (int)t.n, lane), m = extend_cut(pb, sb, (int)t.m, lane);

  const int iE = (int)E, iP = (int)P, stride = 2 * iE + 3, off = iE + 1; // entry d of a row at index d + off: -E - 1 .. E + 1
  int32_t* const rows = s_extend + (size_t)wv * 2u * (uint32_t)stride;
  for (int q = (int)lane; q < 2 * stride; q += 64) rows[q] = EXTEND_NONE;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // (one wave writes and reads its own rows: LDS serves a wave in order)

  // the lane's best entry: e ascends and within a row the lane's d ascends, so a later entry wins only with a larger S
  int best_s = -0x7FFFFFFF, best_e = 0x7FFFFFFF, best_d = 0x7FFFFFFF;
  for (int e = 0; e <= iE; ++e) {
    int32_t* const cur = rows + (e & 1) * stride;
    const int32_t* const prev = rows + ((e & 1) ^ 1) * stride;
    const int dlo = -e > -n ? -e : -n, dhi = e < m ? e : m; // the row's diagonals: inside the matrix, within e of the main one
    for (int base = dlo; base <= dhi; base += 64) {         // (the same trips for every lane)
      const int d = base + (int)lane;
      if (d <= dhi) {
        const int lo = d < 0 ? -d : 0, hi = n < m - d ? n : m - d; // the rows of diagonal d inside the matrix: lo <= hi for -n <= d <= m
        int32_t cand = EXTEND_NONE;
        if (e == 0) {
          cand = 0; // (dlo = dhi = 0)
        } else {
          const int32_t stay = prev[d + off], right = prev[d + 1 + off], left = prev[d - 1 + off]; // (indices 0 .. 2 E + 2)
          if (stay >= 0) cand = stay + 1 <= hi ? stay + 1 : stay;
          if (right >= 0 && right + 1 >= lo && right + 1 <= hi && right + 1 > cand) cand = right + 1;
          if (left >= lo && left <= hi && left > cand) cand = left;
        }
        if (cand >= 0) {
          while (cand < hi) { // (cand >= lo: cand + d >= 0; cand < hi: both positions inside the cut strings, so both codes are 0 .. 3)
            const uint8_t ca = pa[sa * cand], cb = pb[sb * (cand + d)];
            if (ca != (comp ? (uint8_t)(3u - cb) : cb)) break;
            ++cand;
          }
          const int s = 2 * cand + d - iP * e;
          if (s > best_s) {
            best_s = s;
            best_e = e;
            best_d = d;
          }
        }
        cur[d + off] = cand;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    int wave_s = best_s;
    for (int x = 32; x >= 1; x >>= 1) {
      const int other = __shfl_xor(wave_s, x);
      wave_s = other > wave_s ? other : wave_s;
    }
    if (n + m - iP * (e + 1) <= wave_s) break; // (the same for every lane: an entry of a later row has S <= n + m - P (e + 1), and a larger e)
  }
  // the wave's best: S descending, then e ascending, then d ascending
  for (int x = 32; x >= 1; x >>= 1) {
    const int os = __shfl_xor(best_s, x), oe = __shfl_xor(best_e, x), od = __shfl_xor(best_d, x);
    if (os > best_s || (os == best_s && (oe < best_e || (oe == best_e && od < best_d)))) {
      best_s = os;
      best_e = oe;
      best_d = od;
    }
  }
  if (lane == 0) {
    const int i = (best_s + iP * best_e - best_d) / 2; // (row 0 always has its entry: S = 2 i + d - P e of a real one)
    out[w] = { (uint32_t)i, (uint32_t)(i + best_d), (uint32_t)best_e, (uint32_t)n, (uint32_t)m };
  }
}

int edit_extend_run(nts_ctx* ctx, const nts_genome* ga, const nts_genome* gb, const nts_extend_task* tasks, uint64_t n, uint32_t penalty,
                    uint32_t max_edits, nts_extend_result* out)
{
  if (n > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_edit_extend: 2^32 tasks or more");
  std::vector<ExtendTask> prepared(n);
  for (uint64_t i = 0; i < n; ++i) {
    const nts_extend_task& t = tasks[i];
    if (t.n > EXTEND_MAX_LEN || t.m > EXTEND_MAX_LEN) return fail(ctx, NTS_EINVAL, "nts_edit_extend: task " + std::to_string(i) + " asks for more than 65535 bases");
    if (t.flags & ~(NTS_EXTEND_A_BACKWARDS | NTS_EXTEND_B_BACKWARDS | NTS_EXTEND_B_COMPLEMENT))
      return fail(ctx, NTS_EINVAL, "nts_edit_extend: task " + std::to_string(i) + " has unknown flag bits");
    if (t.rec_a >= ga->n_rec || t.rec_b >= gb->n_rec) return fail(ctx, NTS_EINVAL, "nts_edit_extend: task " + std::to_string(i) + ": record index out of range");
    // a string stays inside its record: forwards pos + n <= rec_len, backwards n <= pos + 1 <= rec_len; n = 0 reads nothing (pos <= rec_len)
    auto inside = [](uint64_t pos, uint32_t len, bool backwards, uint64_t rec_len) {
      if (pos > rec_len) return false;
      if (len == 0) return true;
      return backwards ? pos < rec_len && len <= pos + 1 : len <= rec_len - pos;
    };
    if (!inside(t.pos_a, t.n, t.flags & NTS_EXTEND_A_BACKWARDS, ga->rec_len[t.rec_a]) || !inside(t.pos_b, t.m, t.flags & NTS_EXTEND_B_BACKWARDS, gb->rec_len[t.rec_b]))
      return fail(ctx, NTS_EINVAL, "nts_edit_extend: task " + std::to_string(i) + ": a string leaves its record");
    prepared[i] = { ga->rec_off[t.rec_a] + t.pos_a, gb->rec_off[t.rec_b] + t.pos_b, t.n, t.m, t.flags, 0u };
  }
  if (n == 0) return NTS_OK;
  NTS_WS(d_tasks, ExtendTask*, "extend_tasks", n * sizeof(ExtendTask));
  NTS_WS(d_out, nts_extend_result*, "extend_out", n * sizeof(nts_extend_result));
  hipError_t e = hipMemcpyAsync(d_tasks, prepared.data(), n * sizeof(ExtendTask), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_out, 0, n * sizeof(nts_extend_result), ctx->stream);
  if (e == hipSuccess) {
    ScopedTimer t(ctx, "edit_extend", true);
    const size_t lds = (size_t)EXTEND_WAVES * 2u * (2u * max_edits + 3u) * sizeof(int32_t);
    NTS_LAUNCH(k_edit_extend, dim3((uint32_t)((n + EXTEND_WAVES - 1) / EXTEND_WAVES)), dim3(EXTEND_WAVES * 64), lds, ctx->stream,
               (const uint8_t*)ga->d_code + PAD, (const uint8_t*)gb->d_code + PAD, (const ExtendTask*)d_tasks, n, penalty, max_edits, d_out);
    e = hipGetLastError();
  }
  std::vector<nts_extend_result> got(n); // (the caller's array is written only by a call that succeeds)
  if (e == hipSuccess) e = hipMemcpyAsync(got.data(), d_out, n * sizeof(nts_extend_result), hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t e_sync = hipStreamSynchronize(ctx->stream); // (whatever happened: `prepared` was the source of an asynchronous copy)
  HIP_TRY(ctx, e);
  HIP_TRY(ctx, e_sync);
  memcpy(out, got.data(), n * sizeof(nts_extend_result));
  return NTS_OK;
}

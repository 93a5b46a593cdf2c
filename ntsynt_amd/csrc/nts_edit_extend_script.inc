// ---- the edit script of an extended flank (nts_edit_extend_script; ntsynt_amd/assess.py block_ends with_variants) ----
// docs/design/04_21_block_end_variants.md.  Input: the tasks of nts_edit_extend and its results.  For task t, A' = the first ext_a bases
// of its string A as nts_edit_extend reads it (forwards or backwards from pos_a), B' = the first ext_b bases of its string B as read
// (forwards or backwards, complemented or not), D = results[t].edits.  Output: for every task with D >= 1 the D ops of the canonical
// script of A' and B' (docs/design/04_17_block_variants.md) at first[t] .. first[t] + D - 1, p and q offsets in the strings as read.
// Plan (rocprim): an exclusive scan of D over the tasks gives `first`, a selection keeps the tasks with D >= 1, a second scan over the
// kept list gives every member's table offset.  The host cuts the kept list, in order, into batches whose tables fit the budget.
// k_edit_extend_script: one 64-lane wave per member, ESCRIPT_WAVES waves per workgroup, one launch per batch.  Forward: the row update
// of k_edit_wide_script with the task's D -- row e covers d in [max(-e, -n', delta - (D - e)), min(e, m', delta + (D - e))], n' = ext_a,
// m' = ext_b, delta = m' - n' -- read through the task's strides as k_edit_extend reads, the two live rows in LDS (2 Dmax + 3 entries
// each, Dmax the call's largest D), and every finished row also to the member's table in global memory: entry (e, d) at e * e + d + e,
// (D + 1)^2 int32 entries per member, never initialised.  The wave goes on only if F_D[delta] = n' and F_{D-1}[delta] < n'.  Traceback
// from (n', m') as k_edit_wide_script walks.  No atomic, no launch per task, no floating point.

constexpr uint32_t ESCRIPT_WAVES = 2; // 2 waves x 2 rows x (2 Dmax + 3) x 4 B: at most 32 784 B per workgroup (Dmax = 1023)
constexpr int32_t ESCRIPT_NONE = -1;

struct ExtendScriptTask // what the kernel needs of a task and its result: the two first bases, the lengths ext_a and ext_b, the flags, D
{
  uint64_t a0, b0;
  uint32_t n, m, flags, edits;
};
static_assert(sizeof(ExtendScriptTask) == 32, "one task, two 16-byte loads");

struct ExtendScriptCount // what task i adds to the number of ops
{
  const ExtendScriptTask* tasks;
  __host__ __device__ uint64_t operator()(uint32_t i) const { return tasks[i].edits; }
};

struct ExtendScriptKeep // task i has a script
{
  const ExtendScriptTask* tasks;
  __host__ __device__ bool operator()(uint32_t i) const { return tasks[i].edits >= 1u; }
};

struct ExtendScriptTable // the table entries of the kept member w
{
  const uint32_t* kept;
  const ExtendScriptTask* tasks;
  __host__ __device__ uint64_t operator()(uint32_t w) const
  {
    const uint64_t rows = (uint64_t)tasks[kept[w]].edits + 1u;
    return rows * rows;
  }
};

// the diagonals of row e of a member: inside the matrix, within e of the main one, within the D - e edits that remain of delta
__device__ __forceinline__ void escript_range(int e, int n, int m, int delta, int D, int& dlo, int& dhi)
{
  dlo = -e > -n ? -e : -n;
  dhi = e < m ? e : m;
  if (delta - (D - e) > dlo) dlo = delta - (D - e);
  if (delta + (D - e) < dhi) dhi = delta + (D - e);
}

__global__ __launch_bounds__(ESCRIPT_WAVES * 64) void k_edit_extend_script(
  const uint8_t* __restrict__ code_a, const uint8_t* __restrict__ code_b, const ExtendScriptTask* __restrict__ tasks, uint64_t n_tasks, uint32_t Dmax,
  const uint64_t* __restrict__ first, const uint32_t* __restrict__ kept, const uint64_t* __restrict__ n_kept, const uint64_t* __restrict__ tab_off,
  uint64_t w0, uint64_t w1, uint64_t tab_base, uint64_t tab_cap, int32_t* table, nts_edit_op* __restrict__ ops, uint64_t n_ops,
  uint32_t* __restrict__ status)
{
  extern __shared__ int32_t s_escript[]; // ESCRIPT_WAVES x 2 rows x (2 Dmax + 3)
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t w = w0 + (uint64_t)blockIdx.x * ESCRIPT_WAVES + wv; // this batch: the kept members w0 .. w1 - 1
  if (w >= w1) return;
  if (w >= *n_kept) {
    if (lane == 0) status[w] = SCRIPT_OK;
    return;
  }
  const uint32_t tidx = kept[w];
  // (the host refused all of what follows before the launch: a lane still touches nothing outside its strings, rows, table and slots)
  if (tidx >= n_tasks || Dmax < 1u || Dmax > EXTEND_MAX_EDITS) {
    if (lane == 0) status[w] = 0u;
    return;
  }
  const ExtendScriptTask t = tasks[tidx];
  const uint32_t uD = t.edits;
  const uint64_t slot0 = first[tidx], t0 = tab_off[w];
  const uint64_t cells = ((uint64_t)uD + 1u) * ((uint64_t)uD + 1u);
  if (t.n > EXTEND_MAX_LEN || t.m > EXTEND_MAX_LEN || uD < 1u || uD > Dmax || (t.n > t.m ? t.n - t.m : t.m - t.n) > uD || uD > (t.n > t.m ? t.n : t.m) ||
      slot0 > n_ops || uD > n_ops - slot0 || t0 < tab_base || t0 - tab_base > tab_cap || cells > tab_cap - (t0 - tab_base)) {
    if (lane == 0) status[w] = tidx;
    return;
  }
  const int n = (int)t.n, m = (int)t.m, D = (int)uD, delta = m - n;
  int32_t* const tab = table + (t0 - tab_base); // entry (e, d) at e * e + d + e < (e + 1)^2 <= cells
  const uint8_t* const pa = code_a + t.a0;
  const uint8_t* const pb = code_b + t.b0;
  const int64_t sa = (t.flags & NTS_EXTEND_A_BACKWARDS) ? -1 : 1, sb = (t.flags & NTS_EXTEND_B_BACKWARDS) ? -1 : 1;
  const bool comp = (t.flags & NTS_EXTEND_B_COMPLEMENT) != 0;

  // every base of both strings once: after this pass every code is 0 .. 3, the slides and the traceback may complement with 3 - c
  bool bad = false;
  for (int p = (int)lane; p < n; p += 64) bad |= pa[sa * p] >= nts::CODE_INVALID;
  for (int q = (int)lane; q < m; q += 64) bad |= pb[sb * q] >= nts::CODE_INVALID;
  if (__any(bad)) {
    if (lane == 0) status[w] = tidx;
    return;
  }

  const int stride = 2 * (int)Dmax + 3, off = (int)Dmax + 1; // entry d of a row at index d + off: -Dmax - 1 .. Dmax + 1 (|d| <= D <= Dmax)
  int32_t* const rows = s_escript + (size_t)wv * 2u * (uint32_t)stride;
  for (int q = (int)lane; q < 2 * stride; q += 64) rows[q] = ESCRIPT_NONE;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // (one wave writes and reads its own rows: LDS serves a wave in order)

  // forward: rows 0 .. D, each to LDS for the next row and to the table for the traceback
  int32_t end_d = ESCRIPT_NONE, end_less = ESCRIPT_NONE; // F_D[delta] and F_{D-1}[delta], on the lane that computed them
  for (int e = 0; e <= D; ++e) {
    int32_t* const cur = rows + (e & 1) * stride;
    const int32_t* const prev = rows + ((e & 1) ^ 1) * stride;
    int dlo, dhi;
    escript_range(e, n, m, delta, D, dlo, dhi);
    for (int base = dlo; base <= dhi; base += 64) { // (the same trips for every lane)
      const int d = base + (int)lane;
      if (d <= dhi) {
        const int lo = d < 0 ? -d : 0, hi = n < m - d ? n : m - d; // the rows of diagonal d inside the matrix: lo <= hi for -n <= d <= m
        int32_t cand = ESCRIPT_NONE;
        if (e == 0) {
          cand = 0; // (dlo = dhi = 0)
        } else {
          const int32_t stay = prev[d + off], right = prev[d + 1 + off], left = prev[d - 1 + off]; // (indices 0 .. 2 Dmax + 2)
          if (stay >= 0) cand = stay + 1 <= hi ? stay + 1 : stay;
          if (right >= 0 && right + 1 >= lo && right + 1 <= hi && right + 1 > cand) cand = right + 1;
          if (left >= lo && left <= hi && left > cand) cand = left;
        }
        if (cand >= 0) {
          while (cand < hi) { // (cand >= lo: cand + d >= 0; cand < hi: both positions inside A' and B')
            const uint8_t ca = pa[sa * cand], cb = pb[sb * (cand + d)];
            if (ca != (comp ? (uint8_t)(3u - cb) : cb)) break;
            ++cand;
          }
        }
        cur[d + off] = cand;
        tab[e * e + d + e] = cand; // (-e <= d <= e: consecutive lanes, consecutive entries)
        if (d == delta && e == D) end_d = cand;
        if (d == delta && e == D - 1) end_less = cand;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
  // consistency: D edits reach the corner, D - 1 do not (where row D - 1 does not hold delta, |delta| = D: they cannot)
  if (!__any(end_d == n) || __any(end_less >= n)) {
    if (lane == 0) status[w] = tidx;
    return;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // the last row's stores before the first table read (one wave, its own table)

  // traceback, the whole wave at one cell (i, j) of value e
  int i = n, j = m, e = D;
  bool broken = false;
  while (i > 0 || j > 0) {
    nts_edit_op op{ tidx, 0u, 0u, 0u, 0xFFu, 0xFFu, 0u };
    if (i > 0 && j > 0) {
      const int k = (int)lane;
      bool eq = false;
      if (i - 1 - k >= 0 && j - 1 - k >= 0) {
        const uint8_t ca = pa[sa * (i - 1 - k)], cb = pb[sb * (j - 1 - k)];
        eq = ca == (comp ? (uint8_t)(3u - cb) : cb);
      }
      const uint64_t differ = ~__ballot(eq);
      const int run = differ ? __builtin_ctzll(differ) : 64;
      i -= run;
      j -= run;
      if (run == 64 || i == 0 || j == 0) continue;
      if (e == 0) {
        broken = true;
        break;
      }
      // lane 0 reads F_{e-1}[d], lane 1 F_{e-1}[d + 1]: "none" outside row e - 1's written range
      const int d = j - i, dq = d + (int)(lane & 1u);
      int dlo, dhi;
      escript_range(e - 1, n, m, delta, D, dlo, dhi);
      int32_t f = ESCRIPT_NONE;
      if (lane < 2u && dq >= dlo && dq <= dhi) f = tab[(e - 1) * (e - 1) + dq + (e - 1)]; // (dlo >= -(e - 1), dhi <= e - 1: inside row e - 1)
      const uint64_t reach = __ballot(f >= i - 1);
      if (reach & 1ull) {
        op.op = NTS_OP_SUB, op.p = (uint32_t)(i - 1), op.q = (uint32_t)(j - 1);
        --i, --j;
      } else if (reach & 2ull) {
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
      if (op.op != NTS_OP_INS) op.base_a = pa[sa * (int64_t)op.p]; // (p < n')
      if (op.op != NTS_OP_DEL) {                                   // (q < m')
        const uint8_t cb = pb[sb * (int64_t)op.q];
        op.base_b = comp ? (uint8_t)(3u - cb) : cb;
      }
      ops[slot0 + (uint32_t)e - 1u] = op; // (1 <= e <= D: a slot of this task)
    }
    --e;
  }
  if (lane == 0) status[w] = (broken || e != 0) ? tidx : SCRIPT_OK;
}

int edit_extend_script_run(nts_ctx* ctx, const nts_genome* ga, const nts_genome* gb, const nts_extend_task* tasks, uint64_t n,
                           const nts_extend_result* results, uint64_t table_budget, nts_edit_op** ops, uint64_t* n_ops, uint64_t* first)
{
  ctx->last_escript_members = ctx->last_escript_table_bytes = ctx->last_escript_batches = 0;
  if (n > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_edit_extend_script: 2^32 tasks or more");
  const uint64_t budget = table_budget ? table_budget : NTS_WIDE_SCRIPT_TABLE_BUDGET;
  std::vector<ExtendScriptTask> prepared(n);
  uint32_t d_max = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const nts_extend_task& t = tasks[i];
    const nts_extend_result& r = results[i];
    const std::string who = "nts_edit_extend_script: task " + std::to_string(i);
    if (t.n > EXTEND_MAX_LEN || t.m > EXTEND_MAX_LEN) return fail(ctx, NTS_EINVAL, who + " asks for more than 65535 bases");
    if (t.flags & ~(NTS_EXTEND_A_BACKWARDS | NTS_EXTEND_B_BACKWARDS | NTS_EXTEND_B_COMPLEMENT)) return fail(ctx, NTS_EINVAL, who + " has unknown flag bits");
    if (t.rec_a >= ga->n_rec || t.rec_b >= gb->n_rec) return fail(ctx, NTS_EINVAL, who + ": record index out of range");
    // (nts_edit_extend's test: forwards pos + n <= rec_len, backwards n <= pos + 1 <= rec_len; n = 0 reads nothing, pos <= rec_len)
    auto inside = [](uint64_t pos, uint32_t len, bool backwards, uint64_t rec_len) {
      if (pos > rec_len) return false;
      if (len == 0) return true;
      return backwards ? pos < rec_len && len <= pos + 1 : len <= rec_len - pos;
    };
    if (!inside(t.pos_a, t.n, t.flags & NTS_EXTEND_A_BACKWARDS, ga->rec_len[t.rec_a]) || !inside(t.pos_b, t.m, t.flags & NTS_EXTEND_B_BACKWARDS, gb->rec_len[t.rec_b]))
      return fail(ctx, NTS_EINVAL, who + ": a string leaves its record");
    if (r.ext_a > t.n || r.ext_b > t.m) return fail(ctx, NTS_EINVAL, who + ": its result extends beyond the task's strings");
    if (r.edits > EXTEND_MAX_EDITS) return fail(ctx, NTS_EINVAL, who + ": its result has more than 1023 edits");
    if (r.edits < (r.ext_a > r.ext_b ? r.ext_a - r.ext_b : r.ext_b - r.ext_a))
      return fail(ctx, NTS_EINVAL, who + ": its result's edits are below the difference of its lengths");
    if (r.edits > std::max(r.ext_a, r.ext_b)) return fail(ctx, NTS_EINVAL, who + ": its result's edits are above the longer of its lengths");
    prepared[i] = { ga->rec_off[t.rec_a] + t.pos_a, gb->rec_off[t.rec_b] + t.pos_b, r.ext_a, r.ext_b, t.flags, r.edits };
    d_max = std::max(d_max, r.edits);
  }
  if (budget < 4ull * (d_max + 1ull) * (d_max + 1ull))
    return fail(ctx, NTS_EINVAL, "nts_edit_extend_script: table_budget below 4 (Dmax + 1)^2 bytes, the largest table of one task");
  // the ops and the tables; the batches: members in index order while their tables fit the budget
  uint64_t total = 0, kept = 0, bytes_all = 0, bytes_batch = 0, bytes_most = 0;
  std::vector<uint64_t> cut{ 0 }, cut_entries{ 0 }; // batch b: kept members cut[b] .. cut[b + 1] - 1, its tables from entry cut_entries[b]
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t d = prepared[i].edits;
    if (d == 0) continue;
    const uint64_t bytes = 4ull * (d + 1ull) * (d + 1ull); // (<= 4 (Dmax + 1)^2 <= budget: a member alone always fits)
    if (bytes_batch + bytes > budget) {
      cut.push_back(kept);
      cut_entries.push_back(bytes_all / 4);
      bytes_batch = 0;
    }
    bytes_batch += bytes;
    bytes_most = std::max(bytes_most, bytes_batch);
    bytes_all += bytes;
    total += d;
    ++kept;
  }
  cut.push_back(kept);
  cut_entries.push_back(bytes_all / 4);
  if (total > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_edit_extend_script: 2^32 edits or more");
  *ops = nullptr;
  *n_ops = 0;
  if (first) memset(first, 0, (n + 1) * 8);
  if (n == 0 || kept == 0) return NTS_OK; // (no task with an edit: every `first` entry is 0, nothing is launched)
  ctx->last_escript_members = kept;
  ctx->last_escript_table_bytes = bytes_all;
  ctx->last_escript_batches = cut.size() - 1;
  NTS_WS(d_tasks, ExtendScriptTask*, "escript_tasks", n * sizeof(ExtendScriptTask));
  NTS_WS(d_first, uint64_t*, "edit_first", n * 8);
  NTS_WS(d_kept, uint32_t*, "edit_kept", n * 4);
  NTS_WS(d_taboff, uint64_t*, "edit_taboff", kept * 8);
  NTS_WS(d_status, uint32_t*, "edit_status", kept * 4);
  NTS_WS(d_num, uint64_t*, "edit_num", 8);
  NTS_WS(d_worst, uint32_t*, "edit_worst", 4);
  NTS_WS(d_ops, nts_edit_op*, "edit_ops", total * sizeof(nts_edit_op));
  const WideScriptTables tables_block(ctx, bytes_most); // (bytes_most <= budget; released when the call ends)
  int32_t* const d_table = tables_block.p;
  if (!d_table) return NTS_ENOMEM;
  hipError_t e = hipMemcpyAsync(d_tasks, prepared.data(), n * sizeof(ExtendScriptTask), hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) hipStreamSynchronize(ctx->stream); // (before `prepared` goes away)
  HIP_TRY(ctx, e);
  nts_edit_op* host_ops = nullptr;
  std::vector<uint64_t> host_first(first ? n : 0); // (the caller's array keeps its zeros unless the call succeeds)
  uint32_t worst = SCRIPT_OK;
  hipError_t e_run = hipSuccess;
  {
    ScopedTimer t(ctx, "edit_extend_script_plan");
    auto counts = rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0), ExtendScriptCount{ d_tasks });
    auto flags = rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0), ExtendScriptKeep{ d_tasks });
    auto tables = rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0), ExtendScriptTable{ d_kept, d_tasks });
    size_t tmp_scan = 0, tmp_sel = 0, tmp_tab = 0;
    e_run = rocprim::exclusive_scan(nullptr, tmp_scan, counts, d_first, (uint64_t)0, n, rocprim::plus<uint64_t>(), ctx->stream);
    if (e_run == hipSuccess)
      e_run = rocprim::select(nullptr, tmp_sel, rocprim::counting_iterator<uint32_t>(0), flags, d_kept, d_num, n, ctx->stream);
    if (e_run == hipSuccess)
      e_run = rocprim::exclusive_scan(nullptr, tmp_tab, tables, d_taboff, (uint64_t)0, kept, rocprim::plus<uint64_t>(), ctx->stream);
    void* d_tmp = e_run == hipSuccess ? ws_get(ctx, "ivs_tmp", std::max<size_t>(std::max(tmp_scan, std::max(tmp_sel, tmp_tab)), 16)) : nullptr;
    if (e_run == hipSuccess && !d_tmp) e_run = hipErrorOutOfMemory;
    if (e_run == hipSuccess) e_run = rocprim::exclusive_scan(d_tmp, tmp_scan, counts, d_first, (uint64_t)0, n, rocprim::plus<uint64_t>(), ctx->stream);
    if (e_run == hipSuccess) e_run = rocprim::select(d_tmp, tmp_sel, rocprim::counting_iterator<uint32_t>(0), flags, d_kept, d_num, n, ctx->stream);
    // (the host counted `kept` with the same predicate: the selection wrote exactly that many indices)
    if (e_run == hipSuccess) e_run = rocprim::exclusive_scan(d_tmp, tmp_tab, tables, d_taboff, (uint64_t)0, kept, rocprim::plus<uint64_t>(), ctx->stream);
  }
  if (e_run == hipSuccess) {
    {
      ScopedTimer t(ctx, "edit_extend_script", true);
      const size_t lds = (size_t)ESCRIPT_WAVES * 2u * (2u * d_max + 3u) * sizeof(int32_t);
      for (size_t b = 0; b + 1 < cut.size(); ++b) { // (one stream: a batch's tables are free again when the next batch starts)
        const uint64_t members = cut[b + 1] - cut[b];
        NTS_LAUNCH(k_edit_extend_script, dim3((uint32_t)((members + ESCRIPT_WAVES - 1) / ESCRIPT_WAVES)), dim3(ESCRIPT_WAVES * 64), lds, ctx->stream,
                   (const uint8_t*)ga->d_code + PAD, (const uint8_t*)gb->d_code + PAD, (const ExtendScriptTask*)d_tasks, n, d_max, (const uint64_t*)d_first,
                   (const uint32_t*)d_kept, (const uint64_t*)d_num, (const uint64_t*)d_taboff, cut[b], cut[b + 1], cut_entries[b],
                   cut_entries[b + 1] - cut_entries[b], d_table, d_ops, total, d_status);
      }
      size_t tmp = 0;
      e_run = rocprim::reduce(nullptr, tmp, d_status, d_worst, SCRIPT_OK, kept, ScriptMin(), ctx->stream);
      void* d_tmp = e_run == hipSuccess ? ws_get(ctx, "ivs_tmp", std::max<size_t>(tmp, 16)) : nullptr;
      if (e_run == hipSuccess && !d_tmp) e_run = hipErrorOutOfMemory;
      if (e_run == hipSuccess) e_run = rocprim::reduce(d_tmp, tmp, d_status, d_worst, SCRIPT_OK, kept, ScriptMin(), ctx->stream);
    }
    if (e_run == hipSuccess) e_run = hipGetLastError();
    if (e_run == hipSuccess) e_run = hipMemcpyAsync(&worst, d_worst, 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e_run == hipSuccess) {
      host_ops = (nts_edit_op*)malloc(total * sizeof(nts_edit_op));
      if (host_ops) e_run = hipMemcpyAsync(host_ops, d_ops, total * sizeof(nts_edit_op), hipMemcpyDeviceToHost, ctx->stream); // all batches, one copy
    }
  }
  if (e_run == hipSuccess && first) e_run = hipMemcpyAsync(host_first.data(), d_first, n * 8, hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t e_sync = hipStreamSynchronize(ctx->stream); // (whatever happened: `prepared` was the source of an asynchronous copy)
  if (e_run != hipSuccess || e_sync != hipSuccess || worst != SCRIPT_OK) {
    free(host_ops);
    host_ops = nullptr;
  }
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  if (worst != SCRIPT_OK) return fail(ctx, NTS_EINVAL, "nts_edit_extend_script: results is not the extension of task " + std::to_string(worst));
  if (!host_ops) return fail(ctx, NTS_ENOMEM, "nts_edit_extend_script: no host memory for the ops");
  if (first) memcpy(first, host_first.data(), n * 8);
  if (first) first[n] = total;
  *ops = host_ops;
  *n_ops = total;
  return NTS_OK;
}

// ---- the edit script of an extended flank (nts_edit_extend_script; ntsynt_amd/assess.py block_ends with_variants) ----
// docs/design/04_21_block_end_variants.md.  Input: the tasks of nts_edit_extend and its results.  For task t, A' = the first ext_a bases
// of its string A as nts_edit_extend reads it (forwards or backwards from pos_a), B' = the first ext_b bases of its string B as read
// (forwards or backwards, complemented or not), D = results[t].edits.  Output: for every task with D >= 1 the D ops of the canonical
// script of A' and B' (docs/design/04_17_block_variants.md) at first[t] .. first[t] + D - 1, p and q offsets in the strings as read.
// Plan (rocprim): an exclusive scan of D over the tasks gives `first`, a selection keeps the tasks with D >= 1, a second scan over the
// kept list gives every member's table offset.  The host cuts the kept list, in order, into batches whose tables fit the budget.
// k_edit_extend_script: one 64-lane wave per member, FR_WAVES waves per workgroup, one launch per batch; the kernel fetches and checks
// its member, fr_script_wave (csrc/nts_edit_fr_script.inc) does the rest through a TaskReader.  Forward: the row update
// of k_edit_wide_script with the task's D -- row e covers d in [max(-e, -n', delta - (D - e)), min(e, m', delta + (D - e))], n' = ext_a,
// m' = ext_b, delta = m' - n' -- read through the task's strides as k_edit_extend reads, the two live rows in LDS (2 Dmax + 3 entries
// each, Dmax the call's largest D), and every finished row also to the member's table in global memory: entry (e, d) at e * e + d + e,
// (D + 1)^2 int32 entries per member, never initialised.  The wave goes on only if F_D[delta] = n' and F_{D-1}[delta] < n'.  Traceback
// from (n', m') as k_edit_wide_script walks.  No atomic, no launch per task, no floating point.

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

__global__ __launch_bounds__(FR_WAVES * 64) void k_edit_extend_script(
  const uint8_t* __restrict__ code_a, const uint8_t* __restrict__ code_b, const ExtendScriptTask* __restrict__ tasks, uint64_t n_tasks, uint32_t Dmax,
  const uint64_t* __restrict__ first, const uint32_t* __restrict__ kept, const uint64_t* __restrict__ n_kept, const uint64_t* __restrict__ tab_off,
  uint64_t w0, uint64_t w1, uint64_t tab_base, uint64_t tab_cap, int32_t* table, nts_edit_op* __restrict__ ops, uint64_t n_ops,
  uint32_t* __restrict__ status)
{
  extern __shared__ int32_t s_escript[]; // FR_WAVES x 2 rows x (2 Dmax + 3)
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t w = w0 + (uint64_t)blockIdx.x * FR_WAVES + wv; // this batch: the kept members w0 .. w1 - 1
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
  const TaskReader rd{ code_a + t.a0, code_b + t.b0, (t.flags & NTS_EXTEND_A_BACKWARDS) ? -1 : 1, (t.flags & NTS_EXTEND_B_BACKWARDS) ? -1 : 1,
                       (t.flags & NTS_EXTEND_B_COMPLEMENT) != 0 };
  const int stride = 2 * (int)Dmax + 3, off = (int)Dmax + 1; // entry d of a row at index d + off: -Dmax - 1 .. Dmax + 1 (|d| <= D <= Dmax)
  // A' and B' of n' = t.n and m' = t.m bases; the member's table: entry (e, d) at e * e + d + e < (e + 1)^2 <= cells
  const uint32_t st = fr_script_wave(rd, (int)t.n, (int)t.m, (int)uD, s_escript + (size_t)wv * 2u * (uint32_t)stride, stride, off, table + (t0 - tab_base), ops + slot0,
                                     tidx, lane);
  if (lane == 0) status[w] = st;
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
  ScriptBatches bt(budget);
  for (uint64_t i = 0; i < n; ++i)
    if (prepared[i].edits) bt.add(prepared[i].edits); // (4 (d + 1)^2 <= 4 (Dmax + 1)^2 <= budget)
  bt.close();
  const uint64_t total = bt.total, kept = bt.kept;
  if (total > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_edit_extend_script: 2^32 edits or more");
  *ops = nullptr;
  *n_ops = 0;
  if (first) memset(first, 0, (n + 1) * 8);
  if (n == 0 || kept == 0) return NTS_OK; // (no task with an edit: every `first` entry is 0, nothing is launched)
  ctx->last_escript_members = kept;
  ctx->last_escript_table_bytes = bt.bytes_all;
  ctx->last_escript_batches = bt.batches();
  NTS_WS(d_tasks, ExtendScriptTask*, "escript_tasks", n * sizeof(ExtendScriptTask));
  NTS_WS(d_first, uint64_t*, "edit_first", n * 8);
  NTS_WS(d_kept, uint32_t*, "edit_kept", n * 4);
  NTS_WS(d_taboff, uint64_t*, "edit_taboff", kept * 8);
  NTS_WS(d_status, uint32_t*, "edit_status", kept * 4);
  NTS_WS(d_num, uint64_t*, "edit_num", 8);
  NTS_WS(d_worst, uint32_t*, "edit_worst", 4);
  NTS_WS(d_ops, nts_edit_op*, "edit_ops", total * sizeof(nts_edit_op));
  const ScriptTables tables_block(ctx, bt.bytes_most); // (bytes_most <= budget; released when the call ends)
  int32_t* const d_table = tables_block.p;
  if (!d_table) return NTS_ENOMEM;
  hipError_t e = hipMemcpyAsync(d_tasks, prepared.data(), n * sizeof(ExtendScriptTask), hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) hipStreamSynchronize(ctx->stream); // (before `prepared` goes away)
  HIP_TRY(ctx, e);
  std::vector<uint64_t> host_first(first ? n : 0); // (the caller's array keeps its zeros unless the call succeeds)
  const rocprim::counting_iterator<uint32_t> index(0);
  const hipError_t e_plan = script_plan(ctx, "edit_extend_script_plan", rocprim::make_transform_iterator(index, ExtendScriptCount{ d_tasks }),
                                        rocprim::make_transform_iterator(index, ExtendScriptKeep{ d_tasks }), n, d_first, d_kept, d_num,
                                        rocprim::make_transform_iterator(index, ExtendScriptTable{ d_kept, d_tasks }), kept, d_taboff);
  auto launch = [&] {
    for (size_t b = 0; b < bt.batches(); ++b)
      NTS_LAUNCH(k_edit_extend_script, dim3(bt.grid(b)), dim3(FR_WAVES * 64), fr_rows_bytes(d_max), ctx->stream, (const uint8_t*)ga->d_code + PAD,
                 (const uint8_t*)gb->d_code + PAD, (const ExtendScriptTask*)d_tasks, n, d_max, (const uint64_t*)d_first, (const uint32_t*)d_kept,
                 (const uint64_t*)d_num, (const uint64_t*)d_taboff, bt.cut[b], bt.cut[b + 1], bt.cut_entries[b], bt.cut_entries[b + 1] - bt.cut_entries[b],
                 d_table, d_ops, total, d_status);
  };
  ScriptDone done;
  if (int rc = script_finish(ctx, e_plan, "edit_extend_script", launch, d_status, d_worst, kept, d_ops, total, d_first, first ? host_first.data() : nullptr, n, done))
    return rc;
  if (done.worst != SCRIPT_OK) return fail(ctx, NTS_EINVAL, "nts_edit_extend_script: results is not the extension of task " + std::to_string(done.worst));
  if (done.no_memory) return fail(ctx, NTS_ENOMEM, "nts_edit_extend_script: no host memory for the ops");
  if (first) memcpy(first, host_first.data(), n * 8);
  if (first) first[n] = total;
  *ops = done.ops;
  *n_ops = total;
  return NTS_OK;
}

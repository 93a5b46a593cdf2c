// ---- the edit script of the stretches the 31-diagonal band leaves out (nts_edit_wide_script; ntsynt_amd/assess.py ----
// block_wide_variants).  docs/design/04_19_block_wide_variants.md.  Input: the segments, intervals and flips of nts_edit_wide and its
// dist_out.  The script set: segments with a distance D that nts_edit_script does not take -- kind offband, or a candidate with
// D + |delta| > 2 W + 1.  Output: the D ops of every member's canonical script (docs/design/04_17_block_variants.md) at first[seg] ..
// first[seg] + D - 1.
// Plan (rocprim): an exclusive scan of D over the script set gives `first`, a selection keeps the members' indices, a second scan over
// the kept list gives every member's table offset.  The host cuts the kept list, in order, into batches whose tables fit the budget.
// k_edit_wide_script: one 64-lane wave per member, FR_WAVES waves per workgroup, one launch per batch; the kernel fetches and checks
// its member, fr_script_wave (csrc/nts_edit_fr_script.inc) does the rest through a SegReader.  Forward: k_edit_wide's row
// update with the known D in place of E -- row e covers d in [max(-e, -n, delta - (D - e)), min(e, m, delta + (D - e))], the two live
// rows in LDS, and every finished row also goes to the member's table in global memory: entry (e, d) at e * e + d + e, (D + 1)^2 int32
// entries per member, never initialised.  The wave goes on only if F_D[delta] = n and F_{D-1}[delta] < n.  Traceback from (n, m) as
// k_edit_script walks: a ballot over the 64 positions back along the diagonal gives the match run, at the mismatch F_{e-1}[d] >= i - 1
// selects SUB, else F_{e-1}[d + 1] >= i - 1 DEL, else INS, the two entries read from the table by lanes 0 and 1 -- an entry outside its
// row's written range is "none" by the range test, whatever memory holds.  No atomic, no launch per segment, no floating point.

// segment i belongs to the script set (host and device)
struct WideScriptKeep
{
  const nts_iv_segment* segs;
  const uint32_t* dist;
  uint32_t band;
  __host__ __device__ bool operator()(uint32_t i) const
  {
    const uint32_t d = dist[i];
    if (d >= NTS_EDIT_INVALID) return false;
    if (segs[i].kind == NTS_SEG_OFFBAND) return true;
    if (segs[i].kind != NTS_SEG_CANDIDATE) return false;
    const int64_t delta = (int64_t)segs[i].dy - (int64_t)segs[i].dx;
    return (uint64_t)d + (uint64_t)(delta < 0 ? -delta : delta) > 2ull * band + 1ull;
  }
};

struct WideScriptCount // what segment i adds to the number of ops
{
  WideScriptKeep keep;
  __host__ __device__ uint64_t operator()(uint32_t i) const { return keep(i) ? keep.dist[i] : 0u; }
};

struct WideScriptTable // the table entries of the kept member w
{
  const uint32_t* kept;
  const uint32_t* dist;
  __host__ __device__ uint64_t operator()(uint32_t w) const
  {
    const uint64_t rows = (uint64_t)dist[kept[w]] + 1u;
    return rows * rows;
  }
};

__global__ __launch_bounds__(FR_WAVES * 64) void k_edit_wide_script(
  const uint8_t* __restrict__ code_a, const uint8_t* __restrict__ code_b, const EditIv* __restrict__ ivs, uint64_t n_iv,
  const nts_iv_segment* __restrict__ segs, uint64_t n_segs, uint32_t E, const uint32_t* __restrict__ dist, const uint64_t* __restrict__ first,
  const uint32_t* __restrict__ kept, const uint64_t* __restrict__ n_kept, const uint64_t* __restrict__ tab_off, uint64_t w0, uint64_t w1,
  uint64_t tab_base, uint64_t tab_cap, int32_t* table, nts_edit_op* __restrict__ ops, uint64_t n_ops, uint32_t* __restrict__ status)
{
  extern __shared__ int32_t s_wscript[]; // FR_WAVES x 2 rows x (2 E + 3)
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t w = w0 + (uint64_t)blockIdx.x * FR_WAVES + wv; // this batch: the kept members w0 .. w1 - 1
  if (w >= w1) return;
  if (w >= *n_kept) {
    if (lane == 0) status[w] = SCRIPT_OK;
    return;
  }
  const uint32_t sidx = kept[w];
  // (the host refused all of what follows before the launch: a lane still touches nothing outside its strings, rows, table and slots)
  if (sidx >= n_segs || E < 3u || E > WIDE_MAX_EDITS) {
    if (lane == 0) status[w] = 0u;
    return;
  }
  const nts_iv_segment s = segs[sidx];
  const uint32_t uD = dist[sidx];
  const uint64_t slot0 = first[sidx], t0 = tab_off[w];
  const int n = (int)s.dx, m = s.dy;
  const int delta = m - n, ad = delta < 0 ? -delta : delta;
  EditIv v{ 0, 0, 0, 0, 0, 0 };
  if (s.iv_a < n_iv) v = ivs[s.iv_a];
  const uint64_t cells = ((uint64_t)uD + 1u) * ((uint64_t)uD + 1u);
  if ((s.kind != NTS_SEG_CANDIDATE && s.kind != NTS_SEG_OFFBAND) || n < 1 || m < 1 || n > (int)EDIT_MAX_LEN || m > (int)EDIT_MAX_LEN || uD < 1u || uD > E ||
      (uint32_t)ad > uD || (uint64_t)s.x + (uint32_t)n > v.la || (uint64_t)s.y_lo + (uint32_t)m > v.lb || slot0 > n_ops || uD > n_ops - slot0 ||
      t0 < tab_base || t0 - tab_base > tab_cap || cells > tab_cap - (t0 - tab_base)) {
    if (lane == 0) status[w] = sidx;
    return;
  }
  const bool flip = v.flip != 0;
  const SegReader rd{ code_a + v.a0 + s.x, flip ? code_b + v.b0 + (v.lb - 1u - s.y_lo) : code_b + v.b0 + s.y_lo, flip }; // (as k_edit_wave reads B)
  const int stride = 2 * (int)E + 3, off = (int)E + 1; // entry d of a row at index d + off: -E - 1 .. E + 1 (|d| <= D <= E)
  // the member's table: entry (e, d) at e * e + d + e < (e + 1)^2 <= cells
  const uint32_t st = fr_script_wave(rd, n, m, (int)uD, s_wscript + (size_t)wv * 2u * (uint32_t)stride, stride, off, table + (t0 - tab_base), ops + slot0, sidx, lane);
  if (lane == 0) status[w] = st;
}

int edit_wide_script_run(nts_ctx* ctx, const nts_genome* ga, const nts_genome* gb, const nts_interval* iv_a, const nts_interval* iv_b,
                         const nts_iv_segment* segs, uint64_t n, uint64_t n_iv, const uint8_t* flip, uint32_t band, uint32_t max_edits,
                         const uint32_t* dist, uint64_t table_budget, nts_edit_op** ops, uint64_t* n_ops, uint64_t* first)
{
  *ops = nullptr;
  *n_ops = 0;
  ctx->last_wscript_members = ctx->last_wscript_table_bytes = ctx->last_wscript_batches = 0;
  const uint64_t budget = table_budget ? table_budget : NTS_WIDE_SCRIPT_TABLE_BUDGET;
  if (budget < 4ull * (max_edits + 1ull) * (max_edits + 1ull))
    return fail(ctx, NTS_EINVAL, "nts_edit_wide_script: table_budget below 4 (max_edits + 1)^2 bytes, one member's largest table");
  std::vector<EditIv> ivs;
  if (int rc = edit_prepare(ctx, ga, gb, iv_a, iv_b, segs, n, n_iv, flip, band, ivs)) return rc;
  // the script set, its ops and its tables; the batches: members in index order while their tables fit the budget
  const WideScriptKeep keep{ segs, dist, band };
  ScriptBatches bt(budget);
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t d = dist[i];
    if (d >= NTS_EDIT_INVALID) continue;
    const nts_iv_segment& s = segs[i];
    if (s.kind != NTS_SEG_CANDIDATE && s.kind != NTS_SEG_OFFBAND)
      return fail(ctx, NTS_EINVAL, "nts_edit_wide_script: a distance on segment " + std::to_string(i) + ", which is neither candidate nor offband");
    const int64_t delta = (int64_t)s.dy - (int64_t)s.dx, ad = delta < 0 ? -delta : delta;
    if (d > max_edits) return fail(ctx, NTS_EINVAL, "nts_edit_wide_script: the distance of segment " + std::to_string(i) + " lies beyond max_edits");
    if ((int64_t)d < ad)
      return fail(ctx, NTS_EINVAL, "nts_edit_wide_script: the distance of segment " + std::to_string(i) + " is below the difference of its lengths");
    if (!keep((uint32_t)i)) continue; // (nts_edit_script's: it adds nothing here)
    if (d == 0) // (an offband segment has |delta| > band >= 1 and so D >= 1; a candidate member D > band + 1)
      return fail(ctx, NTS_EINVAL, "nts_edit_wide_script: a distance of 0 on segment " + std::to_string(i) + ", which is offband: every member has D >= 1");
    if (s.kind == NTS_SEG_OFFBAND) { // (a candidate: edit_prepare checked it)
      const EditIv& v = ivs[s.iv_a];
      if (s.dx < 1 || s.dy < 1 || s.dx > EDIT_MAX_LEN || s.dy > (int32_t)EDIT_MAX_LEN || (uint64_t)s.x + s.dx > v.la || (uint64_t)s.y_lo + (uint32_t)s.dy > v.lb)
        return fail(ctx, NTS_EINVAL, "nts_edit_wide_script: an offband segment of the script set leaves its interval or the length limit");
    }
    bt.add(d); // (4 (d + 1)^2 <= 4 (E + 1)^2 <= budget)
  }
  bt.close();
  const uint64_t total = bt.total, kept = bt.kept;
  if (total > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_edit_wide_script: 2^32 edits or more");
  if (first) memset(first, 0, (n + 1) * 8);
  if (first) first[n] = total;
  if (n == 0 || kept == 0) return NTS_OK; // (an empty script set: every `first` entry is 0, nothing is launched)
  ctx->last_wscript_members = kept;
  ctx->last_wscript_table_bytes = bt.bytes_all;
  ctx->last_wscript_batches = bt.batches();
  NTS_WS(d_ivs, EditIv*, "edit_ivs", std::max<size_t>(n_iv, 1) * sizeof(EditIv));
  NTS_WS(d_seg, nts_iv_segment*, "edit_seg", n * sizeof(nts_iv_segment));
  NTS_WS(d_dist, uint32_t*, "edit_dist", n * 4);
  NTS_WS(d_first, uint64_t*, "edit_first", n * 8);
  NTS_WS(d_kept, uint32_t*, "edit_kept", n * 4);
  NTS_WS(d_taboff, uint64_t*, "edit_taboff", kept * 8);
  NTS_WS(d_status, uint32_t*, "edit_status", kept * 4);
  NTS_WS(d_num, uint64_t*, "edit_num", 8);
  NTS_WS(d_worst, uint32_t*, "edit_worst", 4);
  NTS_WS(d_ops, nts_edit_op*, "edit_ops", total * sizeof(nts_edit_op));
  const ScriptTables tables_block(ctx, bt.bytes_most); // (bytes_most <= budget)
  int32_t* const d_table = tables_block.p;
  if (!d_table) return NTS_ENOMEM;
  hipError_t e = hipMemcpyAsync(d_ivs, ivs.data(), n_iv * sizeof(EditIv), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_seg, segs, n * sizeof(nts_iv_segment), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_dist, dist, n * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) hipStreamSynchronize(ctx->stream); // (before `ivs` goes away)
  HIP_TRY(ctx, e);
  const WideScriptKeep d_keep{ d_seg, d_dist, band };
  const rocprim::counting_iterator<uint32_t> index(0);
  const hipError_t e_plan = script_plan(ctx, "edit_wide_script_plan", rocprim::make_transform_iterator(index, WideScriptCount{ d_keep }),
                                        rocprim::make_transform_iterator(index, d_keep), n, d_first, d_kept, d_num,
                                        rocprim::make_transform_iterator(index, WideScriptTable{ d_kept, d_dist }), kept, d_taboff);
  auto launch = [&] {
    for (size_t b = 0; b < bt.batches(); ++b)
      NTS_LAUNCH(k_edit_wide_script, dim3(bt.grid(b)), dim3(FR_WAVES * 64), fr_rows_bytes(max_edits), ctx->stream, (const uint8_t*)ga->d_code + PAD,
                 (const uint8_t*)gb->d_code + PAD, (const EditIv*)d_ivs, n_iv, (const nts_iv_segment*)d_seg, n, max_edits, (const uint32_t*)d_dist,
                 (const uint64_t*)d_first, (const uint32_t*)d_kept, (const uint64_t*)d_num, (const uint64_t*)d_taboff, bt.cut[b], bt.cut[b + 1],
                 bt.cut_entries[b], bt.cut_entries[b + 1] - bt.cut_entries[b], d_table, d_ops, total, d_status);
  };
  ScriptDone done;
  if (int rc = script_finish(ctx, e_plan, "edit_wide_script", launch, d_status, d_worst, kept, d_ops, total, d_first, first, n, done)) return rc;
  if (done.worst != SCRIPT_OK) return fail(ctx, NTS_EINVAL, "nts_edit_wide_script: dist is not the distance of segment " + std::to_string(done.worst));
  if (done.no_memory) return fail(ctx, NTS_ENOMEM, "nts_edit_wide_script: no host memory for the ops");
  *ops = done.ops;
  *n_ops = total;
  return NTS_OK;
}

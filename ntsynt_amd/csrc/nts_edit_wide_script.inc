// ---- the edit script of the stretches the 31-diagonal band leaves out (nts_edit_wide_script; ntsynt_amd/assess.py ----
// block_wide_variants).  docs/design/04_19_block_wide_variants.md.  Input: the segments, intervals and flips of nts_edit_wide and its
// dist_out.  The script set: segments with a distance D that nts_edit_script does not take -- kind offband, or a candidate with
// D + |delta| > 2 W + 1.  Output: the D ops of every member's canonical script (docs/design/04_17_block_variants.md) at first[seg] ..
// first[seg] + D - 1.
// Plan (rocprim): an exclusive scan of D over the script set gives `first`, a selection keeps the members' indices, a second scan over
// the kept list gives every member's table offset.  The host cuts the kept list, in order, into batches whose tables fit the budget.
// k_edit_wide_script: one 64-lane wave per member, WSCRIPT_WAVES waves per workgroup, one launch per batch.  Forward: k_edit_wide's row
// update with the known D in place of E -- row e covers d in [max(-e, -n, delta - (D - e)), min(e, m, delta + (D - e))], the two live
// rows in LDS, and every finished row also goes to the member's table in global memory: entry (e, d) at e * e + d + e, (D + 1)^2 int32
// entries per member, never initialised.  The wave goes on only if F_D[delta] = n and F_{D-1}[delta] < n.  Traceback from (n, m) as
// k_edit_script walks: a ballot over the 64 positions back along the diagonal gives the match run, at the mismatch F_{e-1}[d] >= i - 1
// selects SUB, else F_{e-1}[d + 1] >= i - 1 DEL, else INS, the two entries read from the table by lanes 0 and 1 -- an entry outside its
// row's written range is "none" by the range test, whatever memory holds.  No atomic, no launch per segment, no floating point.

constexpr uint32_t WSCRIPT_WAVES = 2; // the LDS of k_edit_wide: 2 waves x 2 rows x (2 E + 3) x 4 B
constexpr int32_t WSCRIPT_NONE = -1;

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

// the diagonals of row e of a member: inside the matrix, within e of the main one, within the D - e edits that remain of delta
__device__ __forceinline__ void wscript_range(int e, int n, int m, int delta, int D, int& dlo, int& dhi)
{
  dlo = -e > -n ? -e : -n;
  dhi = e < m ? e : m;
  if (delta - (D - e) > dlo) dlo = delta - (D - e);
  if (delta + (D - e) < dhi) dhi = delta + (D - e);
}

__global__ __launch_bounds__(WSCRIPT_WAVES * 64) void k_edit_wide_script(
  const uint8_t* __restrict__ code_a, const uint8_t* __restrict__ code_b, const EditIv* __restrict__ ivs, uint64_t n_iv,
  const nts_iv_segment* __restrict__ segs, uint64_t n_segs, uint32_t E, const uint32_t* __restrict__ dist, const uint64_t* __restrict__ first,
  const uint32_t* __restrict__ kept, const uint64_t* __restrict__ n_kept, const uint64_t* __restrict__ tab_off, uint64_t w0, uint64_t w1,
  uint64_t tab_base, uint64_t tab_cap, int32_t* table, nts_edit_op* __restrict__ ops, uint64_t n_ops, uint32_t* __restrict__ status)
{
  extern __shared__ int32_t s_wscript[]; // WSCRIPT_WAVES x 2 rows x (2 E + 3)
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t w = w0 + (uint64_t)blockIdx.x * WSCRIPT_WAVES + wv; // this batch: the kept members w0 .. w1 - 1
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
  const int D = (int)uD;
  int32_t* const tab = table + (t0 - tab_base); // entry (e, d) at e * e + d + e < (e + 1)^2 <= cells
  const uint8_t* const pa = code_a + v.a0 + s.x;
  const bool flip = v.flip != 0;
  const uint8_t* const pb = flip ? code_b + v.b0 + (v.lb - 1u - s.y_lo) : code_b + v.b0 + s.y_lo; // (as k_edit_wave reads B)

  // every base of both strings once: after this pass the slides and the traceback compare raw codes
  bool bad = false;
  for (int p = (int)lane; p < n; p += 64) bad |= pa[p] >= nts::CODE_INVALID;
  for (int q = (int)lane; q < m; q += 64) bad |= (flip ? pb[-(int64_t)q] : pb[q]) >= nts::CODE_INVALID;
  if (__any(bad)) {
    if (lane == 0) status[w] = sidx;
    return;
  }

  const int stride = 2 * (int)E + 3, off = (int)E + 1; // entry d of a row at index d + off: -E - 1 .. E + 1 (|d| <= D <= E)
  int32_t* const rows = s_wscript + (size_t)wv * 2u * (uint32_t)stride;
  for (int q = (int)lane; q < 2 * stride; q += 64) rows[q] = WSCRIPT_NONE;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // (one wave writes and reads its own rows: LDS serves a wave in order)

  // forward: rows 0 .. D, each to LDS for the next row and to the table for the traceback
  int32_t end_d = WSCRIPT_NONE, end_less = WSCRIPT_NONE; // F_D[delta] and F_{D-1}[delta], on the lane that computed them
  for (int e = 0; e <= D; ++e) {
    int32_t* const cur = rows + (e & 1) * stride;
    const int32_t* const prev = rows + ((e & 1) ^ 1) * stride;
    int dlo, dhi;
    wscript_range(e, n, m, delta, D, dlo, dhi);
    for (int base = dlo; base <= dhi; base += 64) { // (the same trips for every lane)
      const int d = base + (int)lane;
      if (d <= dhi) {
        const int lo = d < 0 ? -d : 0, hi = n < m - d ? n : m - d; // the rows of diagonal d inside the matrix: lo <= hi for -n <= d <= m
        int32_t cand = WSCRIPT_NONE;
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
        tab[e * e + d + e] = cand; // (-e <= d <= e: consecutive lanes, consecutive entries)
        if (d == delta && e == D) end_d = cand;
        if (d == delta && e == D - 1) end_less = cand;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
  // consistency: D edits reach the corner, D - 1 do not (where row D - 1 does not hold delta, |delta| = D: they cannot)
  if (!__any(end_d == n) || __any(end_less >= n)) {
    if (lane == 0) status[w] = sidx;
    return;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // the last row's stores before the first table read (one wave, its own table)

  // traceback, the whole wave at one cell (i, j) of value e
  int i = n, j = m, e = D;
  bool broken = false;
  while (i > 0 || j > 0) {
    nts_edit_op op{ sidx, 0u, 0u, 0u, 0xFFu, 0xFFu, 0u };
    if (i > 0 && j > 0) {
      const int k = (int)lane;
      bool eq = false;
      if (i - 1 - k >= 0 && j - 1 - k >= 0) {
        const uint8_t ca = pa[i - 1 - k], cb = flip ? (uint8_t)(3u - pb[-(int64_t)(j - 1 - k)]) : pb[j - 1 - k];
        eq = ca == cb;
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
      wscript_range(e - 1, n, m, delta, D, dlo, dhi);
      int32_t f = WSCRIPT_NONE;
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
      if (op.op != NTS_OP_INS) op.base_a = pa[op.p];                                                          // (p < n)
      if (op.op != NTS_OP_DEL) op.base_b = flip ? (uint8_t)(3u - pb[-(int64_t)op.q]) : pb[op.q]; // (q < m)
      ops[slot0 + (uint32_t)e - 1u] = op; // (1 <= e <= D: a slot of this segment)
    }
    --e;
  }
  if (lane == 0) status[w] = (broken || e != 0) ? sidx : SCRIPT_OK;
}

// the block that holds the tables of one call: exactly `bytes` bytes (at most the call's budget), given back to the library's
// allocation cache when the call ends, so that up to 1 GiB does not stay with the context through the later stages of a run
struct WideScriptTables
{
  nts_ctx* ctx;
  int32_t* p = nullptr;
  WideScriptTables(nts_ctx* c, size_t bytes) : ctx(c)
  {
    void* q = nullptr;
    const hipError_t e = dev_malloc(&q, std::max<size_t>(bytes, 256));
    if (e != hipSuccess)
      ctx->err = std::string("hipMalloc 'edit_wide_tables': ") + hipGetErrorString(e);
    else
      p = (int32_t*)q;
  }
  ~WideScriptTables()
  {
    if (p) (void)dev_free(p); // (every return behind the launches has synchronised the stream; dev_free waits for the device itself)
  }
  WideScriptTables(const WideScriptTables&) = delete;
  WideScriptTables& operator=(const WideScriptTables&) = delete;
};

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
  uint64_t total = 0, kept = 0, bytes_all = 0, bytes_batch = 0, bytes_most = 0;
  std::vector<uint64_t> cut{ 0 }, cut_entries{ 0 }; // batch b: kept members cut[b] .. cut[b + 1] - 1, its tables from entry cut_entries[b]
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
    const uint64_t bytes = 4ull * (d + 1ull) * (d + 1ull); // (<= 4 (E + 1)^2 <= budget: a member alone always fits)
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
  if (total > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_edit_wide_script: 2^32 edits or more");
  if (first) memset(first, 0, (n + 1) * 8);
  if (first) first[n] = total;
  if (n == 0 || kept == 0) return NTS_OK; // (an empty script set: every `first` entry is 0, nothing is launched)
  ctx->last_wscript_members = kept;
  ctx->last_wscript_table_bytes = bytes_all;
  ctx->last_wscript_batches = cut.size() - 1;
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
  const WideScriptTables tables_block(ctx, bytes_most); // (bytes_most <= budget)
  int32_t* const d_table = tables_block.p;
  if (!d_table) return NTS_ENOMEM;
  hipError_t e = hipMemcpyAsync(d_ivs, ivs.data(), n_iv * sizeof(EditIv), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_seg, segs, n * sizeof(nts_iv_segment), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_dist, dist, n * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) hipStreamSynchronize(ctx->stream); // (before `ivs` goes away)
  HIP_TRY(ctx, e);
  nts_edit_op* host_ops = nullptr;
  uint32_t worst = SCRIPT_OK;
  hipError_t e_run = hipSuccess;
  {
    ScopedTimer t(ctx, "edit_wide_script_plan");
    const WideScriptKeep d_keep{ d_seg, d_dist, band };
    auto counts = rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0), WideScriptCount{ d_keep });
    auto flags = rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0), d_keep);
    auto tables = rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0), WideScriptTable{ d_kept, d_dist });
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
      ScopedTimer t(ctx, "edit_wide_script", true);
      const size_t lds = (size_t)WSCRIPT_WAVES * 2u * (2u * max_edits + 3u) * sizeof(int32_t);
      for (size_t b = 0; b + 1 < cut.size(); ++b) { // (one stream: a batch's tables are free again when the next batch starts)
        const uint64_t members = cut[b + 1] - cut[b];
        NTS_LAUNCH(k_edit_wide_script, dim3((uint32_t)((members + WSCRIPT_WAVES - 1) / WSCRIPT_WAVES)), dim3(WSCRIPT_WAVES * 64), lds, ctx->stream,
                   (const uint8_t*)ga->d_code + PAD, (const uint8_t*)gb->d_code + PAD, (const EditIv*)d_ivs, n_iv, (const nts_iv_segment*)d_seg, n, max_edits,
                   (const uint32_t*)d_dist, (const uint64_t*)d_first, (const uint32_t*)d_kept, (const uint64_t*)d_num, (const uint64_t*)d_taboff, cut[b],
                   cut[b + 1], cut_entries[b], cut_entries[b + 1] - cut_entries[b], d_table, d_ops, total, d_status);
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
  if (e_run == hipSuccess && first) e_run = hipMemcpyAsync(first, d_first, n * 8, hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t e_sync = hipStreamSynchronize(ctx->stream); // (whatever happened: `ivs` was the source of an asynchronous copy)
  if (e_run != hipSuccess || e_sync != hipSuccess || worst != SCRIPT_OK) {
    free(host_ops);
    host_ops = nullptr;
  }
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  if (worst != SCRIPT_OK) return fail(ctx, NTS_EINVAL, "nts_edit_wide_script: dist is not the distance of segment " + std::to_string(worst));
  if (!host_ops) return fail(ctx, NTS_ENOMEM, "nts_edit_wide_script: no host memory for the ops");
  *ops = host_ops;
  *n_ops = total;
  return NTS_OK;
}

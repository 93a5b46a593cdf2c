// ---- what the three edit-script calls share (nts_edit_script, nts_edit_wide_script, nts_edit_extend_script) ----
// docs/design/04_17_block_variants.md, 04_19_block_wide_variants.md, 04_21_block_end_variants.md.  Device: fr_script_wave, the
// furthest-reaching wave body of k_edit_wide_script and k_edit_extend_script, which read their bases through SegReader and TaskReader.
// (k_edit_script keeps its own body: a 64 x 64 table in static LDS, one lane per diagonal, invalid bases met lazily.)  Host:
// ScriptBatches cuts the members into batches of tables, script_plan runs the rocPRIM plan, script_finish launches, reduces and copies.
// Known differences between the callers that callers and tests see; they stay in the drivers and are not unified here:
//   - after a run that fails behind the launch, nts_edit_wide_script has written the caller's `first` (zeros, then first[n] = total);
//     nts_edit_extend_script stages `first` on the host and leaves the caller's array zeroed;
//   - nts_edit_wide_script clears *ops / *n_ops before any check, nts_edit_extend_script only after its checks pass;
//   - nts_edit_script writes first[n] and returns early for n = 0; for kept = 0 it runs its plan, launches nothing and gives *ops = NULL;
//   - nts_edit_wide_script tests table_budget before edit_prepare, nts_edit_extend_script after its task loop;
//   - nts_edit_script reports missing host memory ahead of a wrong dist, the other two the other way round.

constexpr int32_t FR_NONE = -1;
constexpr uint32_t FR_WAVES = 2; // the table kernels: 2 waves x 2 rows x (2 Dmax + 3) x 4 B of LDS, at most 32 784 B per workgroup (Dmax = 1023)
constexpr uint32_t SCRIPT_OK = 0xFFFFFFFFu;

struct ScriptMin
{
  __host__ __device__ uint32_t operator()(uint32_t x, uint32_t y) const { return x < y ? x : y; }
};

// A[p] and B[q] of a segment as k_edit_wave reads them: B backwards from pb and complemented where the interval is flipped.  a_raw and
// b_raw for the validity pass; a and b the codes as compared (valid codes only)
struct SegReader
{
  const uint8_t *pa, *pb;
  bool flip;
  __device__ __forceinline__ uint8_t a_raw(int p) const { return pa[p]; }
  __device__ __forceinline__ uint8_t b_raw(int q) const { return flip ? pb[-(int64_t)q] : pb[q]; }
  __device__ __forceinline__ uint8_t a(int p) const { return pa[p]; }
  __device__ __forceinline__ uint8_t b(int q) const { return flip ? (uint8_t)(3u - pb[-(int64_t)q]) : pb[q]; }
};

// A[p] and B[q] of a task as k_edit_extend reads them: each string forwards or backwards (stride 1 or -1), B complemented or not
struct TaskReader
{
  const uint8_t *pa, *pb;
  int64_t sa, sb;
  bool comp;
  __device__ __forceinline__ uint8_t a_raw(int p) const { return pa[sa * p]; }
  __device__ __forceinline__ uint8_t b_raw(int q) const { return pb[sb * q]; }
  __device__ __forceinline__ uint8_t a(int p) const { return pa[sa * p]; }
  __device__ __forceinline__ uint8_t b(int q) const
  {
    const uint8_t cb = pb[sb * q];
    return comp ? (uint8_t)(3u - cb) : cb;
  }
};

// the diagonals of row e of a member: inside the matrix, within e of the main one, within the D - e edits that remain of delta
__device__ __forceinline__ void fr_row_range(int e, int n, int m, int delta, int D, int& dlo, int& dhi)
{
  dlo = -e > -n ? -e : -n;
  dhi = e < m ? e : m;
  if (delta - (D - e) > dlo) dlo = delta - (D - e);
  if (delta + (D - e) < dhi) dhi = delta + (D - e);
}

// One wave, one member: the canonical script of A[0 .. n) and B[0 .. m) at distance D, op e - 1 to ops[e - 1] with op.seg = id.  The
// caller checked 0 <= n, m; |m - n| <= D <= max(n, m); the strings, the D slots of `ops` and the (D + 1)^2 entries of `tab` inside their buffers;
// `rows` = the wave's two LDS rows of `stride` entries, entry d of a row at index d + off, |d| <= D < off, off + D + 1 < stride.
// Returns what lane 0 stores as the member's status: SCRIPT_OK, or id where a base is invalid or D is not the distance.
template <class Reader>
__device__ __forceinline__ uint32_t fr_script_wave(const Reader rd, const int n, const int m, const int D, int32_t* const rows, const int stride, const int off,
                                                   int32_t* const tab, nts_edit_op* const ops, const uint32_t id, const uint32_t lane)
{
  const int delta = m - n;
  // every base of both strings once: after this pass every code is 0 .. 3, the slides and the traceback may complement with 3 - c
  bool bad = false;
  for (int p = (int)lane; p < n; p += 64) bad |= rd.a_raw(p) >= nts::CODE_INVALID;
  for (int q = (int)lane; q < m; q += 64) bad |= rd.b_raw(q) >= nts::CODE_INVALID;
  if (__any(bad)) return id;

  for (int q = (int)lane; q < 2 * stride; q += 64) rows[q] = FR_NONE;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // (one wave writes and reads its own rows: LDS serves a wave in order)

  // forward: rows 0 .. D, each to LDS for the next row and to the table for the traceback
  int32_t end_d = FR_NONE, end_less = FR_NONE; // F_D[delta] and F_{D-1}[delta], on the lane that computed them
  for (int e = 0; e <= D; ++e) {
    int32_t* const cur = rows + (e & 1) * stride;
    const int32_t* const prev = rows + ((e & 1) ^ 1) * stride;
    int dlo, dhi;
    fr_row_range(e, n, m, delta, D, dlo, dhi);
    for (int base = dlo; base <= dhi; base += 64) { // (the same trips for every lane)
      const int d = base + (int)lane;
      if (d <= dhi) {
        const int lo = d < 0 ? -d : 0, hi = n < m - d ? n : m - d; // the rows of diagonal d inside the matrix: lo <= hi for -n <= d <= m
        int32_t cand = FR_NONE;
        if (e == 0) {
          cand = 0; // (dlo = dhi = 0)
        } else {
          const int32_t stay = prev[d + off], right = prev[d + 1 + off], left = prev[d - 1 + off]; // (indices 0 .. stride - 1)
          if (stay >= 0) cand = stay + 1 <= hi ? stay + 1 : stay;
          if (right >= 0 && right + 1 >= lo && right + 1 <= hi && right + 1 > cand) cand = right + 1;
          if (left >= lo && left <= hi && left > cand) cand = left;
        }
        if (cand >= 0) {
          while (cand < hi) { // (cand >= lo: cand + d >= 0; cand < hi: both positions inside the strings)
            if (rd.a(cand) != rd.b(cand + d)) break;
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
  if (!__any(end_d == n) || __any(end_less >= n)) return id;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // the last row's stores before the first table read (one wave, its own table)

  // traceback, the whole wave at one cell (i, j) of value e
  int i = n, j = m, e = D;
  while (i > 0 || j > 0) {
    nts_edit_op op{ id, 0u, 0u, 0u, 0xFFu, 0xFFu, 0u };
    if (i > 0 && j > 0) {
      const int k = (int)lane;
      bool eq = false;
      if (i - 1 - k >= 0 && j - 1 - k >= 0) eq = rd.a(i - 1 - k) == rd.b(j - 1 - k);
      const uint64_t differ = ~__ballot(eq);
      const int run = differ ? __builtin_ctzll(differ) : 64;
      i -= run;
      j -= run;
      if (run == 64 || i == 0 || j == 0) continue;
      if (e == 0) return id;
      // lane 0 reads F_{e-1}[d], lane 1 F_{e-1}[d + 1]: "none" outside row e - 1's written range, whatever memory holds
      const int d = j - i, dq = d + (int)(lane & 1u);
      int dlo, dhi;
      fr_row_range(e - 1, n, m, delta, D, dlo, dhi);
      int32_t f = FR_NONE;
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
    if (e == 0) return id;
    if (lane == 0) {
      if (op.op != NTS_OP_INS) op.base_a = rd.a((int)op.p); // (p < n)
      if (op.op != NTS_OP_DEL) op.base_b = rd.b((int)op.q); // (q < m)
      ops[(uint32_t)e - 1u] = op;                           // (1 <= e <= D: a slot of this member)
    }
    --e;
  }
  return e != 0 ? id : SCRIPT_OK;
}

// the block that holds the tables of one call: exactly `bytes` bytes (at most the call's budget), given back to the library's
// allocation cache when the call ends, so that up to 1 GiB does not stay with the context through the later stages of a run
struct ScriptTables
{
  nts_ctx* ctx;
  int32_t* p = nullptr;
  ScriptTables(nts_ctx* c, size_t bytes) : ctx(c)
  {
    void* q = nullptr;
    const hipError_t e = dev_malloc(&q, std::max<size_t>(bytes, 256));
    if (e != hipSuccess)
      ctx->err = std::string("hipMalloc 'edit_wide_tables': ") + hipGetErrorString(e);
    else
      p = (int32_t*)q;
  }
  ~ScriptTables()
  {
    if (p) (void)dev_free(p); // (every return behind the launches has synchronised the stream; dev_free waits for the device itself)
  }
  ScriptTables(const ScriptTables&) = delete;
  ScriptTables& operator=(const ScriptTables&) = delete;
};

// the members of a call, in index order, cut into batches whose tables fit `budget` bytes: add(D) per member (4 (D + 1)^2 <= budget,
// a member alone always fits), close() behind the last.  Batch b: kept members cut[b] .. cut[b + 1] - 1, its tables from entry
// cut_entries[b] of all; bytes_most = the largest batch, what one call allocates
struct ScriptBatches
{
  uint64_t budget, total = 0, kept = 0, bytes_all = 0, bytes_batch = 0, bytes_most = 0;
  std::vector<uint64_t> cut{ 0 }, cut_entries{ 0 };
  explicit ScriptBatches(uint64_t b) : budget(b) {}
  void add(uint64_t d)
  {
    const uint64_t bytes = 4ull * (d + 1ull) * (d + 1ull);
    if (bytes_batch + bytes > budget) {
      close();
      bytes_batch = 0;
    }
    bytes_batch += bytes;
    bytes_most = std::max(bytes_most, bytes_batch);
    bytes_all += bytes;
    total += d;
    ++kept;
  }
  void close()
  {
    cut.push_back(kept);
    cut_entries.push_back(bytes_all / 4);
  }
  size_t batches() const { return cut.size() - 1; }
  uint32_t grid(size_t b) const { return (uint32_t)((cut[b + 1] - cut[b] + FR_WAVES - 1) / FR_WAVES); }
};

constexpr size_t fr_rows_bytes(uint32_t d_max) { return (size_t)FR_WAVES * 2u * (2u * d_max + 3u) * sizeof(int32_t); } // the LDS of a workgroup

struct ScriptNoTable // (nts_edit_script: its table is in LDS)
{
};

// The plan under the timer `timer`, on the stream: an exclusive scan of `counts` over the n members gives d_first, a selection by
// `flags` gives d_kept and *d_num, and, with tables, an exclusive scan of `tables` over the `kept` kept members gives d_taboff (the
// host counted `kept` with the same predicate: the selection wrote exactly that many indices).
template <class Counts, class Flags, class Tables = ScriptNoTable>
hipError_t script_plan(nts_ctx* ctx, const char* timer, Counts counts, Flags flags, uint64_t n, uint64_t* d_first, uint32_t* d_kept, uint64_t* d_num,
                       Tables tables = Tables(), uint64_t kept = 0, uint64_t* d_taboff = nullptr)
{
  constexpr bool with_tables = !std::is_same<Tables, ScriptNoTable>::value;
  ScopedTimer t(ctx, timer);
  const rocprim::counting_iterator<uint32_t> index(0);
  size_t tmp_scan = 0, tmp_sel = 0, tmp_tab = 0;
  hipError_t e_run = rocprim::exclusive_scan(nullptr, tmp_scan, counts, d_first, (uint64_t)0, n, rocprim::plus<uint64_t>(), ctx->stream);
  if (e_run == hipSuccess) e_run = rocprim::select(nullptr, tmp_sel, index, flags, d_kept, d_num, n, ctx->stream);
  if constexpr (with_tables)
    if (e_run == hipSuccess) e_run = rocprim::exclusive_scan(nullptr, tmp_tab, tables, d_taboff, (uint64_t)0, kept, rocprim::plus<uint64_t>(), ctx->stream);
  void* d_tmp = e_run == hipSuccess ? ws_get(ctx, "ivs_tmp", std::max<size_t>(std::max(tmp_scan, std::max(tmp_sel, tmp_tab)), 16)) : nullptr;
  if (e_run == hipSuccess && !d_tmp) e_run = hipErrorOutOfMemory;
  if (e_run == hipSuccess) e_run = rocprim::exclusive_scan(d_tmp, tmp_scan, counts, d_first, (uint64_t)0, n, rocprim::plus<uint64_t>(), ctx->stream);
  if (e_run == hipSuccess) e_run = rocprim::select(d_tmp, tmp_sel, index, flags, d_kept, d_num, n, ctx->stream);
  if constexpr (with_tables)
    if (e_run == hipSuccess) e_run = rocprim::exclusive_scan(d_tmp, tmp_tab, tables, d_taboff, (uint64_t)0, kept, rocprim::plus<uint64_t>(), ctx->stream);
  return e_run;
}

struct ScriptDone // what script_finish hands back: ops is NULL unless everything succeeded and kept >= 1
{
  uint32_t worst = SCRIPT_OK; // the smallest member id whose wave refused it
  nts_edit_op* ops = nullptr; // malloc'ed: the caller's
  bool no_memory = false;     // malloc failed
};

// Behind the plan (e_run: its result).  With kept >= 1, under the timer `timer`: launch() -- the caller's kernel, every batch -- and
// the smallest status; then the `total` ops to new host memory.  In any case d_first[0 .. n) to `first` (where not NULL) and the
// stream synchronised, whatever happened: the caller's staged input was the source of asynchronous copies.  Returns the HIP failure.
template <class Launch>
int script_finish(nts_ctx* ctx, hipError_t e_run, const char* timer, Launch launch, uint32_t* d_status, uint32_t* d_worst, uint64_t kept,
                  const nts_edit_op* d_ops, uint64_t total, const uint64_t* d_first, uint64_t* first, uint64_t n, ScriptDone& done)
{
  if (e_run == hipSuccess && kept) {
    {
      ScopedTimer t(ctx, timer, true);
      launch(); // (one stream: a batch's tables are free again when the next batch starts)
      size_t tmp = 0;
      e_run = rocprim::reduce(nullptr, tmp, d_status, d_worst, SCRIPT_OK, kept, ScriptMin(), ctx->stream);
      void* d_tmp = e_run == hipSuccess ? ws_get(ctx, "ivs_tmp", std::max<size_t>(tmp, 16)) : nullptr;
      if (e_run == hipSuccess && !d_tmp) e_run = hipErrorOutOfMemory;
      if (e_run == hipSuccess) e_run = rocprim::reduce(d_tmp, tmp, d_status, d_worst, SCRIPT_OK, kept, ScriptMin(), ctx->stream);
    }
    if (e_run == hipSuccess) e_run = hipGetLastError();
    if (e_run == hipSuccess) e_run = hipMemcpyAsync(&done.worst, d_worst, 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e_run == hipSuccess) {
      done.ops = (nts_edit_op*)malloc(total * sizeof(nts_edit_op));
      done.no_memory = !done.ops;
      if (done.ops) e_run = hipMemcpyAsync(done.ops, d_ops, total * sizeof(nts_edit_op), hipMemcpyDeviceToHost, ctx->stream); // all batches, one copy
    }
  }
  if (e_run == hipSuccess && first) e_run = hipMemcpyAsync(first, d_first, n * 8, hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t e_sync = hipStreamSynchronize(ctx->stream);
  if (e_run != hipSuccess || e_sync != hipSuccess || done.worst != SCRIPT_OK) {
    free(done.ops);
    done.ops = nullptr;
  }
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  return NTS_OK;
}

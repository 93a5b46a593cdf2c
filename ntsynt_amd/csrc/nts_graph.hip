// libntsynt_hip.so, third translation unit: the minimizer graph (rows C1, C2: nts_graph_build) and the graph stage resident in HBM
// (nts_dgraph.inc: nts_engine_*).  Shared state and helpers: nts_internal.h.
#include "nts_internal.h"

// ---- minimizer graph build (rows C1, C2a, C2b) --------------------------------------------------------
namespace {

// after a stable sort by hash, duplicates of one assembly are adjacent (global element index is
// assembly-major): mark elements whose hash is unique within their assembly and kept by the caller
__global__ __launch_bounds__(256) void k_g_valid(const uint64_t* __restrict__ h_sorted, const uint64_t* __restrict__ idx_sorted,
                                                 const uint32_t* __restrict__ asm_of, const uint8_t* __restrict__ keep, uint64_t n,
                                                 uint8_t* __restrict__ valid)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t h = h_sorted[i];
  const uint64_t e = idx_sorted[i];
  const uint32_t a = asm_of[e];
  bool dup = false;
  if (i > 0 && h_sorted[i - 1] == h && asm_of[idx_sorted[i - 1]] == a) dup = true;
  if (i + 1 < n && h_sorted[i + 1] == h && asm_of[idx_sorted[i + 1]] == a) dup = true;
  valid[i] = (!dup && keep[e]) ? 1 : 0;
}

// group heads (first element of each run of equal hashes): the hash is common iff exactly n_asm
// valid elements carry it (each assembly contributes at most one)
__global__ __launch_bounds__(256) void k_g_common(const uint64_t* __restrict__ h_sorted, const uint8_t* __restrict__ valid, uint64_t n,
                                                  uint32_t n_asm, uint64_t* __restrict__ head_common)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t flag = 0;
  const uint64_t h = h_sorted[i];
  if (i == 0 || h_sorted[i - 1] != h) {
    uint32_t cnt = 0;
    for (uint64_t j = i; j < n && h_sorted[j] == h; ++j) cnt += valid[j];
    flag = (cnt == n_asm) ? 1 : 0;
  }
  head_common[i] = flag;
}

__global__ __launch_bounds__(256) void k_g_edge_heads(const uint64_t* __restrict__ key_sorted, uint64_t m, uint64_t* __restrict__ head)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint64_t kk = key_sorted[i];
  head[i] = (kk != ~0ULL && (i == 0 || key_sorted[i - 1] != kk)) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_g_edges(const uint64_t* __restrict__ key_sorted, const uint64_t* __restrict__ seq_sorted,
                                                 const uint64_t* __restrict__ head, const uint64_t* __restrict__ head_scan, uint64_t m,
                                                 const uint32_t* __restrict__ c_vid, uint32_t* __restrict__ e_u, uint32_t* __restrict__ e_v,
                                                 uint32_t* __restrict__ e_w, uint64_t* __restrict__ e_first)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m || !head[i]) return;
  const uint64_t kk = key_sorted[i];
  uint32_t cnt = 0;
  for (uint64_t j = i; j < m && key_sorted[j] == kk; ++j) ++cnt;
  const uint64_t e = head_scan[i];
  const uint64_t s = seq_sorted[i]; // stable sort: the first sighting leads its group
  e_u[e] = c_vid[s];
  e_v[e] = c_vid[s + 1];
  e_w[e] = cnt;
  e_first[e] = s;
}

// ---- edge order of the reference: `[(s, t) for s in edges for t in edges[s]]` over ntJoin's dict of dicts ----
// sources by the time they first became a source, then by creation time; both are sequence numbers < 2^32
__global__ __launch_bounds__(256) void k_g_src_rank(const uint32_t* __restrict__ e_u, const uint64_t* __restrict__ e_first, uint64_t ne,
                                                    unsigned long long* __restrict__ src_rank)
{
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < ne) atomicMin(&src_rank[e_u[e]], (unsigned long long)e_first[e]);
}

__global__ __launch_bounds__(256) void k_g_permute_edges(const uint64_t* __restrict__ idx_sorted, uint64_t ne, const uint32_t* __restrict__ e_u,
                                                         const uint32_t* __restrict__ e_v, const uint32_t* __restrict__ e_w,
                                                         const uint64_t* __restrict__ e_first, uint32_t* __restrict__ o_u,
                                                         uint32_t* __restrict__ o_v, uint32_t* __restrict__ o_w, uint64_t* __restrict__ o_first)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ne) return;
  const uint64_t e = idx_sorted[i];
  o_u[i] = e_u[e];
  o_v[i] = e_v[e];
  o_w[i] = e_w[e];
  o_first[i] = e_first[e];
}

template <typename T>
T* host_copy(nts_ctx* ctx, const T* d, uint64_t n)
{
  T* h = (T*)malloc(std::max<uint64_t>(n, 1) * sizeof(T));
  if (h && n) hipMemcpyAsync(h, d, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream);
  return h;
}

// number of set flags = scan[n-1] + flag[n-1] (scan: the flags' exclusive scan)
int flag_count(nts_ctx* ctx, const uint64_t* flag, const uint64_t* scan, uint64_t n, uint64_t* count)
{
  *count = 0;
  if (n == 0) return NTS_OK;
  uint64_t a = 0, b = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&a, flag + (n - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(&b, scan + (n - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *count = a + b;
  return NTS_OK;
}

// Device-side result of one build, in the context's scratch (valid until the next build on this context)
struct GraphDev
{
  uint64_t n = 0;   // elements given
  uint64_t nv = 0, ne = 0;
  uint64_t* v_hash = nullptr; // [nv] ascending
  uint32_t* occ_rec = nullptr; // [n_asm * nv]
  uint64_t* occ_pos = nullptr;
  uint32_t *e_u = nullptr, *e_v = nullptr, *e_w = nullptr; // [ne] dict order
  uint64_t* e_first = nullptr;
};

// Hook between duplicate removal and the cross-assembly intersection: given valid[e] per element (in element order),
// a caller may rewrite the list ids (refinement rounds cut lists between consecutive *kept* minimizers, row C11).
struct ListHook
{
  virtual int operator()(nts_ctx* ctx, uint64_t n, const uint8_t* d_valid_elem, const uint32_t* d_asm, const uint32_t* d_rec, const uint64_t* d_pos,
                         uint32_t* d_list) = 0;
  virtual ~ListHook() {}
};

__global__ __launch_bounds__(256) void k_g_valid_scatter(const uint64_t* __restrict__ idx_sorted, const uint8_t* __restrict__ valid, uint64_t n,
                                                         uint8_t* __restrict__ valid_elem)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) valid_elem[idx_sorted[i]] = valid[i];
}

// ---- the build: three passes, each over a list of key ranges (slices) ------------------------------------------------------------
// Vertex ids are ranks in ascending hash order.  The elements whose hashes fall into one contiguous range of hash values are
// deduplicated, intersected and numbered on their own: the slices, taken in range order and numbered on from the vertices of the
// slices before them, give the vertices.  A slice holds whole hash values (k_g_valid / k_g_common look at the neighbours with an
// equal hash).  Edges are sliced by their smaller end (the pair key's upper half) and the dict-order sort by the rank of the edge's
// source: both keys order the whole, so the slices' results, one after the other, are in order.
// When the slice buffers of all n elements fit the budget, each pass has one range that holds every item: its members are the
// numbers 0 .. count-1 as they stand, so nothing is counted or selected to plan it, and its buffers stay cached on the context.
// What stays n-sized: the input columns (g_h, g_asm, g_rec, g_pos, g_keep, g_list: 29 B per element), the elements' vertex ids
// (g_evid, 4 B), the valid mask the refinement hook reads (g_valid_elem, 1 B) and the hook's own scan (16 B).  Survivor-sized: the
// survivors' columns (12 B), the unordered edges (20 B per edge; sized by the adjacent pairs when there are several ranges) and the
// results.  Everything else is sized to the largest slice; a build of several ranges gives that and the survivor-sized
// intermediates back at its end, and the hook's scan before its edge pass.

constexpr uint32_t HIST_BINS = 65536;
constexpr uint32_t HIST_CHUNK = 65535; // elements one workgroup counts: a bin's count fits the 16-bit half of an LDS word

// 16-bit bins of a key: counted in LDS (two bins per 32-bit word), one global add per non-empty bin and workgroup
template <typename Key>
__global__ __launch_bounds__(256) void k_g_hist(Key key, uint64_t n, unsigned long long* __restrict__ hist)
{
  __shared__ uint32_t bins[HIST_BINS / 2];
  for (uint32_t b = threadIdx.x; b < HIST_BINS / 2; b += blockDim.x) bins[b] = 0;
  __syncthreads();
  const uint64_t i0 = (uint64_t)blockIdx.x * HIST_CHUNK;
  const uint64_t i1 = n - i0 < HIST_CHUNK ? n : i0 + HIST_CHUNK;
  for (uint64_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
    uint32_t b = 0;
    if (key(i, &b)) atomicAdd(&bins[b >> 1], 1u << ((b & 1u) * 16));
  }
  __syncthreads();
  for (uint32_t w = threadIdx.x; w < HIST_BINS / 2; w += blockDim.x) {
    const uint32_t v = bins[w];
    if (v & 0xFFFFu) atomicAdd(&hist[2 * w], (unsigned long long)(v & 0xFFFFu));
    if (v >> 16) atomicAdd(&hist[2 * w + 1], (unsigned long long)(v >> 16));
  }
}

// adjacent survivors c, c + 1 of one list -> the edge occurrence's canonical key (smaller end in the upper half); others get ~0
__device__ inline uint64_t g_pair_key(const uint32_t* c_vid, const uint32_t* c_asm, const uint32_t* c_list, uint64_t m, uint64_t c)
{
  if (c + 1 < m && c_asm[c] == c_asm[c + 1] && c_list[c] == c_list[c + 1]) {
    const uint64_t u = c_vid[c], v = c_vid[c + 1];
    return u < v ? ((u << 32) | v) : ((v << 32) | u);
  }
  return ~0ULL;
}

// histogram keys (the bin of item i; false: not counted) and slice predicates (item i's key is in [lo, hi])
struct HashBin
{
  const uint64_t* h;
  uint64_t lo, hi;
  uint32_t shift;
  __device__ bool operator()(uint64_t i, uint32_t* b) const
  {
    const uint64_t x = h[i];
    *b = (uint32_t)(x >> shift) & 0xFFFFu;
    return x >= lo && x <= hi;
  }
};
struct HashIn
{
  const uint64_t* h;
  uint64_t lo, hi;
  __device__ bool operator()(uint64_t i) const { return h[i] >= lo && h[i] <= hi; }
};
struct KeptIn
{
  const uint32_t* evid;
  __device__ bool operator()(uint64_t i) const { return evid[i] != 0xFFFFFFFFu; }
};
struct PairBin
{
  const uint32_t *vid, *asm_id, *list;
  uint64_t m;
  uint32_t shift;
  __device__ bool operator()(uint64_t c, uint32_t* b) const
  {
    const uint64_t k = g_pair_key(vid, asm_id, list, m, c);
    *b = (uint32_t)((k >> 32) >> shift);
    return k != ~0ULL;
  }
};
struct PairIn
{
  const uint32_t *vid, *asm_id, *list;
  uint64_t m, lo, hi;
  __device__ bool operator()(uint64_t c) const
  {
    const uint64_t k = g_pair_key(vid, asm_id, list, m, c);
    return k != ~0ULL && (k >> 32) >= lo && (k >> 32) <= hi;
  }
};
struct RankBin
{
  const uint32_t* e_u;
  const unsigned long long* srank;
  uint32_t shift;
  __device__ bool operator()(uint64_t e, uint32_t* b) const
  {
    *b = (uint32_t)(srank[e_u[e]] >> shift);
    return true;
  }
};
struct RankIn
{
  const uint32_t* e_u;
  const unsigned long long* srank;
  uint64_t lo, hi;
  __device__ bool operator()(uint64_t e) const { return srank[e_u[e]] >= lo && srank[e_u[e]] <= hi; }
};

__global__ __launch_bounds__(256) void k_g_gather_h(const uint64_t* __restrict__ idx, uint64_t ns, const uint64_t* __restrict__ h,
                                                    uint64_t* __restrict__ out)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < ns) out[i] = h[idx[i]];
}

// vid_scan = exclusive scan of head_common: every valid element of a common group gets vid_off + the group's rank in the slice
__global__ __launch_bounds__(256) void k_g_slice_vid(const uint64_t* __restrict__ h_sorted, const uint64_t* __restrict__ idx_sorted,
                                                     const uint8_t* __restrict__ valid, const uint64_t* __restrict__ head_common,
                                                     const uint64_t* __restrict__ vid_scan, uint64_t ns, uint64_t vid_off,
                                                     uint32_t* __restrict__ elem_vid)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ns) return;
  const uint64_t h = h_sorted[i];
  if (!(i == 0 || h_sorted[i - 1] != h) || !head_common[i]) return;
  const uint32_t vid = (uint32_t)(vid_off + vid_scan[i]);
  for (uint64_t j = i; j < ns && h_sorted[j] == h; ++j)
    if (valid[j]) elem_vid[idx_sorted[j]] = vid;
}

// once every slice is numbered: each element with a vertex writes its hash and its occurrence
__global__ __launch_bounds__(256) void k_g_vertex_tables(const uint32_t* __restrict__ elem_vid, uint64_t n, const uint64_t* __restrict__ h,
                                                         const uint32_t* __restrict__ asm_of, const uint32_t* __restrict__ rec,
                                                         const uint64_t* __restrict__ pos, uint64_t nv, uint64_t* __restrict__ v_hash,
                                                         uint32_t* __restrict__ occ_rec, uint64_t* __restrict__ occ_pos)
{
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const uint32_t vid = elem_vid[e];
  if (vid == 0xFFFFFFFFu) return;
  v_hash[vid] = h[e]; // (one writer per assembly, all with the same value)
  occ_rec[(uint64_t)asm_of[e] * nv + vid] = rec[e];
  occ_pos[(uint64_t)asm_of[e] * nv + vid] = pos[e];
}

__global__ __launch_bounds__(256) void k_g_gather_survivors(const uint64_t* __restrict__ sel, uint64_t m, const uint32_t* __restrict__ elem_vid,
                                                            const uint32_t* __restrict__ asm_of, const uint32_t* __restrict__ list_id,
                                                            uint32_t* __restrict__ c_vid, uint32_t* __restrict__ c_asm, uint32_t* __restrict__ c_list)
{
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= m) return;
  const uint64_t e = sel[c];
  c_vid[c] = elem_vid[e];
  c_asm[c] = asm_of[e];
  c_list[c] = list_id[e];
}

// sort keys of a slice's members; a null member list stands for the numbers 0 .. ms-1 (the range that holds every item)
__global__ __launch_bounds__(256) void k_g_gather_pairs(const uint64_t* __restrict__ seq, uint64_t ms, const uint32_t* __restrict__ c_vid,
                                                        const uint32_t* __restrict__ c_asm, const uint32_t* __restrict__ c_list, uint64_t m,
                                                        uint64_t* __restrict__ key)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < ms) key[i] = g_pair_key(c_vid, c_asm, c_list, m, seq ? seq[i] : i);
}

__global__ __launch_bounds__(256) void k_g_gather_order(const uint64_t* __restrict__ idx, uint64_t ns, const uint32_t* __restrict__ e_u,
                                                        const uint64_t* __restrict__ e_first, const unsigned long long* __restrict__ src_rank,
                                                        uint64_t* __restrict__ key)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ns) return;
  const uint64_t e = idx ? idx[i] : i;
  key[i] = ((uint64_t)src_rank[e_u[e]] << 32) | e_first[e];
}

// scratch buffer `name` back to the allocator (ws_get keeps buffers by name until ws_release)
void ws_drop(nts_ctx* ctx, const char* name)
{
  auto it = ctx->ws.find(name);
  if (it == ctx->ws.end()) return;
  if (it->second.first) {
    hipStreamSynchronize(ctx->stream);
    dev_free(it->second.first);
  }
  ctx->ws.erase(it);
}

// nts_graph_last_plan's scratch figure: library bytes live beyond those live when the call began, highest where sampled
void graph_sample_peak(nts_ctx* ctx)
{
  const uint64_t now = nts_mem::live.load();
  if (now > ctx->graph_live0) ctx->last_graph_peak = std::max(ctx->last_graph_peak, now - ctx->graph_live0);
}

// the buffers sized to a slice, and the planning's
const char* const SLICE_SCRATCH[] = { "gs_h", "gs_idx", "gs_h2", "gs_idx2", "gs_valid", "gs_flag", "gs_scan", "gs_tmp", "gs_sel_tmp", "gs_cnt",
                                      "gs_hist" };

struct KeyRange
{
  uint64_t lo, hi, n; // [lo, hi] of the key, items in it
};

// 16-bit histogram of `key` over n items (host copy)
template <typename Key>
int slice_hist(nts_ctx* ctx, Key key, uint64_t n, std::vector<uint64_t>* out)
{
  NTS_WS(d_hist, unsigned long long*, "gs_hist", HIST_BINS * 8);
  out->assign(HIST_BINS, 0);
  if (n == 0) return NTS_OK;
  HIP_TRY(ctx, hipMemsetAsync(d_hist, 0, HIST_BINS * 8, ctx->stream));
  NTS_LAUNCH(k_g_hist<Key>, dim3((uint32_t)((n + HIST_CHUNK - 1) / HIST_CHUNK)), dim3(256), 0, ctx->stream, key, n, d_hist);
  HIP_TRY(ctx, hipMemcpyAsync(out->data(), d_hist, HIST_BINS * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return NTS_OK;
}

// key ranges of the planned slices, from their first to their last non-empty bin (bin b covers [base + (b << shift),
// base + ((b + 1) << shift) - 1]); empty slices are left out.  *oversize counts the slices of one bin that hold more than `cap` items.
void slice_ranges(const std::vector<uint64_t>& hist, uint64_t cap, uint64_t base, uint32_t shift, std::vector<KeyRange>* out, uint32_t* oversize)
{
  std::vector<uint32_t> cuts(HIST_BINS + 1);
  uint32_t S = 0;
  nts_graph_plan_slices(hist.data(), HIST_BINS, 1, std::max<uint64_t>(cap, 1), cuts.data(), &S);
  for (uint32_t s = 0; s < S; ++s) {
    uint64_t cnt = 0;
    uint32_t first = cuts[s + 1], last = cuts[s];
    for (uint32_t b = cuts[s]; b < cuts[s + 1]; ++b)
      if (hist[b]) {
        cnt += hist[b];
        first = std::min(first, b);
        last = b;
      }
    if (!cnt) continue;
    if (first == last && cnt > cap) ++*oversize;
    out->push_back({ base + ((uint64_t)first << shift), base + ((uint64_t)last << shift) + ((1ULL << shift) - 1), cnt });
  }
}

// members of one slice, ascending (rocprim::select keeps the input order): the numbers i < n with pred(i)
template <typename Pred>
int slice_select(nts_ctx* ctx, Pred pred, uint64_t n, uint64_t* d_out)
{
  NTS_WS(d_cnt, uint64_t*, "gs_cnt", 8);
  auto in = rocprim::make_counting_iterator<uint64_t>(0);
  size_t tmp = 0;
  HIP_TRY(ctx, rocprim::select(nullptr, tmp, in, d_out, d_cnt, n, pred, ctx->stream));
  NTS_WS(d_tmp, void*, "gs_sel_tmp", std::max<size_t>(tmp, 16));
  HIP_TRY(ctx, rocprim::select(d_tmp, tmp, in, d_out, d_cnt, n, pred, ctx->stream));
  return NTS_OK;
}

// the slice buffers, for slices of up to `ns` items (one set serves the vertex, pair and order passes).  h / idx hold a slice's keys
// and members where they are gathered: not for the vertex range that holds every element, which sorts the hash column as it stands
struct SliceBufs
{
  uint64_t *h, *idx, *h2, *idx2, *flag, *scan;
  uint8_t* valid;
  void* tmp;
  size_t tmp_sort, tmp_scan;
};
int slice_bufs(nts_ctx* ctx, uint64_t ns, bool gathered, SliceBufs* b)
{
  ns = std::max<uint64_t>(ns, 1);
  uint64_t *h = nullptr, *idx = nullptr;
  if (gathered) {
    h = (uint64_t*)ws_get(ctx, "gs_h", ns * 8);
    idx = (uint64_t*)ws_get(ctx, "gs_idx", ns * 8);
    if (!h || !idx) return NTS_ENOMEM;
  }
  NTS_WS(h2, uint64_t*, "gs_h2", ns * 8);
  NTS_WS(idx2, uint64_t*, "gs_idx2", ns * 8);
  NTS_WS(flag, uint64_t*, "gs_flag", ns * 8);
  NTS_WS(scan, uint64_t*, "gs_scan", ns * 8);
  NTS_WS(valid, uint8_t*, "gs_valid", ns);
  size_t tmp_sort = 0, tmp_scan = 0;
  HIP_TRY(ctx, rocprim::radix_sort_pairs(nullptr, tmp_sort, (uint64_t*)nullptr, h2, (uint64_t*)nullptr, idx2, ns, 0, 64, ctx->stream));
  HIP_TRY(ctx, rocprim::exclusive_scan(nullptr, tmp_scan, flag, scan, (uint64_t)0, ns, rocprim::plus<uint64_t>(), ctx->stream));
  NTS_WS(tmp, void*, "gs_tmp", std::max<size_t>(std::max(tmp_sort, tmp_scan), 16));
  *b = { h, idx, h2, idx2, flag, scan, valid, tmp, tmp_sort, tmp_scan };
  return NTS_OK;
}

// stable sort of a slice's (key, member) pairs into b.h2 / b.idx2 (the inputs are left alone); a null member list stands for the
// numbers 0 .. ns-1
int slice_sort(nts_ctx* ctx, const SliceBufs& b, const uint64_t* keys, const uint64_t* members, uint64_t ns)
{
  size_t tmp = b.tmp_sort;
  if (members)
    HIP_TRY(ctx, rocprim::radix_sort_pairs(b.tmp, tmp, keys, b.h2, members, b.idx2, ns, 0, 64, ctx->stream));
  else
    HIP_TRY(ctx, rocprim::radix_sort_pairs(b.tmp, tmp, keys, b.h2, rocprim::make_counting_iterator<uint64_t>(0), b.idx2, ns, 0, 64, ctx->stream));
  return NTS_OK;
}

int slice_scan(nts_ctx* ctx, const SliceBufs& b, uint64_t ns)
{
  size_t tmp = b.tmp_scan;
  HIP_TRY(ctx, rocprim::exclusive_scan(b.tmp, tmp, b.flag, b.scan, (uint64_t)0, ns, rocprim::plus<uint64_t>(), ctx->stream));
  return NTS_OK;
}

// the four edge columns for `ne` edges: the pair pass's, in key order ("g_eu0" ...), or the results in dict order ("g_eu" ...)
struct EdgeCols
{
  uint32_t *u, *v, *w;
  uint64_t* first;
};
int edge_cols(nts_ctx* ctx, bool ordered, uint64_t ne, EdgeCols* e)
{
  ne = std::max<uint64_t>(ne, 1);
  NTS_WS(u, uint32_t*, ordered ? "g_eu" : "g_eu0", ne * 4);
  NTS_WS(v, uint32_t*, ordered ? "g_ev" : "g_ev0", ne * 4);
  NTS_WS(w, uint32_t*, ordered ? "g_ew" : "g_ew0", ne * 4);
  NTS_WS(first, uint64_t*, ordered ? "g_ef" : "g_ef0", ne * 8);
  *e = { u, v, w, first };
  return NTS_OK;
}

uint64_t max_range(const std::vector<KeyRange>& r)
{
  uint64_t m = 0;
  for (const KeyRange& x : r) m = std::max(m, x.n);
  return m;
}

// smallest shift that brings every key below `limit` into 16 bits
uint32_t bin_shift(uint64_t limit)
{
  uint32_t s = 0;
  while (limit > 0 && ((limit - 1) >> s) >= HIST_BINS) ++s;
  return s;
}

constexpr uint32_t MAX_REFINED_BINS = 16; // top-16-bit bins over the cap split again on the next 16 bits (one pass over n each)

// The three passes.  Expects the concatenated elements (assembly-major) in the scratch buffers g_h / g_rec / g_pos / g_keep / g_list /
// g_asm (filled by the callers below); leaves the graph in scratch and describes it in `G`.  `cap`: items per slice; with n <= cap
// every pass has the one range that holds all its items (survivors and edges are no more than n).
int graph_build_ranges(nts_ctx* ctx, uint32_t n_asm, uint64_t n, GraphDev* G, ListHook* hook, uint64_t cap)
{
  const bool sliced = n > cap;
  if (sliced)
    for (const char* nm : SLICE_SCRATCH) ws_drop(ctx, nm); // (what an earlier build that fitted left, sized for all its elements)
  NTS_WS(d_h, uint64_t*, "g_h", n * 8);
  NTS_WS(d_asm, uint32_t*, "g_asm", n * 4);
  NTS_WS(d_rec, uint32_t*, "g_rec", n * 4);
  NTS_WS(d_pos, uint64_t*, "g_pos", n * 8);
  NTS_WS(d_keep, uint8_t*, "g_keep", n);
  NTS_WS(d_list, uint32_t*, "g_list", n * 4);
  NTS_WS(d_evid, uint32_t*, "g_evid", n * 4);
  uint8_t* d_valid_elem = nullptr;
  if (hook) {
    NTS_WS(p, uint8_t*, "g_valid_elem", n);
    d_valid_elem = p;
  }
  HIP_TRY(ctx, hipMemsetAsync(d_evid, 0xFF, n * 4, ctx->stream));
  // ---- plan: the top 16 bits of the hash; a bin over the cap is split on the next 16 bits (the first few such bins)
  uint32_t oversize = 0, refined = 0, top_over = 0;
  std::vector<KeyRange> vr;
  if (sliced) {
    std::vector<uint64_t> hist;
    if (int rc = slice_hist(ctx, HashBin{ d_h, 0, ~0ULL, 48 }, n, &hist)) return rc;
    std::vector<KeyRange> top;
    slice_ranges(hist, cap, 0, 48, &top, &top_over);
    for (const KeyRange& r : top) {
      if (r.n > cap && r.hi - r.lo == (1ULL << 48) - 1 && refined < MAX_REFINED_BINS) {
        ++refined;
        std::vector<uint64_t> sub;
        if (int rc = slice_hist(ctx, HashBin{ d_h, r.lo, r.hi, 32 }, n, &sub)) return rc;
        slice_ranges(sub, cap, r.lo, 32, &vr, &oversize);
      } else {
        if (r.n > cap) ++oversize;
        vr.push_back(r);
      }
    }
  } else {
    vr.push_back({ 0, ~0ULL, n });
  }
  // ---- vertices, slice by slice
  SliceBufs b;
  if (int rc = slice_bufs(ctx, max_range(vr), sliced, &b)) return rc;
  uint64_t nv = 0;
  for (const KeyRange& r : vr) {
    const uint64_t ns = r.n;
    const uint32_t sb = (uint32_t)((ns + 255) / 256);
    const uint64_t* members = nullptr;
    if (sliced) {
      if (int rc = slice_select(ctx, HashIn{ d_h, r.lo, r.hi }, n, b.idx)) return rc;
      members = b.idx;
    }
    {
      ScopedTimer t(ctx, "graph_build");
      if (members) {
        NTS_LAUNCH(k_g_gather_h, dim3(sb), dim3(256), 0, ctx->stream, members, ns, d_h, b.h);
      }
      if (int rc = slice_sort(ctx, b, members ? b.h : d_h, members, ns)) return rc;
      NTS_LAUNCH(k_g_valid, dim3(sb), dim3(256), 0, ctx->stream, b.h2, b.idx2, d_asm, d_keep, ns, b.valid);
      if (hook) {
        NTS_LAUNCH(k_g_valid_scatter, dim3(sb), dim3(256), 0, ctx->stream, b.idx2, b.valid, ns, d_valid_elem);
      }
      NTS_LAUNCH(k_g_common, dim3(sb), dim3(256), 0, ctx->stream, b.h2, b.valid, ns, n_asm, b.flag);
      if (int rc = slice_scan(ctx, b, ns)) return rc;
      NTS_LAUNCH(k_g_slice_vid, dim3(sb), dim3(256), 0, ctx->stream, b.h2, b.idx2, b.valid, b.flag, b.scan, ns, nv, d_evid);
    }
    uint64_t nv_s = 0;
    if (int rc = flag_count(ctx, b.flag, b.scan, ns, &nv_s)) return rc;
    nv += nv_s;
  }
  graph_sample_peak(ctx);
  G->nv = nv;
  const uint64_t n_vslices = vr.size();
  // The hook rewrites list ids only (RefineHook: d_list from the valid mask, records and positions), and the vertex pass does not
  // read them: it runs once, after the last slice.  A sliced build keeps the hook's n-sized scan buffers and the slice buffers from
  // being live at the same time.
  if (hook) {
    if (sliced)
      for (const char* nm : SLICE_SCRATCH) ws_drop(ctx, nm);
    if (int rc = (*hook)(ctx, n, d_valid_elem, d_asm, d_rec, d_pos, d_list)) return rc;
    graph_sample_peak(ctx);
    if (sliced)
      for (const char* nm : { "e_hook_a", "e_hook_b", "e_scan_tmp" }) ws_drop(ctx, nm);
  }
  uint64_t n_eslices = 1;
  if (nv) {
    const uint32_t nb = (uint32_t)((n + 255) / 256);
    NTS_WS(d_vhash, uint64_t*, "g_vhash", nv * 8);
    NTS_WS(d_orec, uint32_t*, "g_orec", (uint64_t)n_asm * nv * 4);
    NTS_WS(d_opos, uint64_t*, "g_opos", (uint64_t)n_asm * nv * 8);
    const uint64_t m = (uint64_t)n_asm * nv; // every common hash occurs once per assembly
    const uint32_t mb = (uint32_t)((m + 255) / 256);
    NTS_WS(d_cvid, uint32_t*, "g_cvid", (m + 1) * 4);
    NTS_WS(d_casm, uint32_t*, "g_casm", m * 4);
    NTS_WS(d_clist, uint32_t*, "g_clist", m * 4);
    NTS_WS(d_sel, uint64_t*, "gs_idx", m * 8); // (the survivors' element numbers; a slice buffer again below)
    {
      ScopedTimer t(ctx, "graph_build");
      NTS_LAUNCH(k_g_vertex_tables, dim3(nb), dim3(256), 0, ctx->stream, d_evid, n, d_h, d_asm, d_rec, d_pos, nv, d_vhash, d_orec, d_opos);
    }
    // survivors in traversal order
    if (int rc = slice_select(ctx, KeptIn{ d_evid }, n, d_sel)) return rc;
    {
      ScopedTimer t(ctx, "graph_build");
      NTS_LAUNCH(k_g_gather_survivors, dim3(mb), dim3(256), 0, ctx->stream, d_sel, m, d_evid, d_asm, d_list, d_cvid, d_casm, d_clist);
    }
    G->v_hash = d_vhash;
    G->occ_rec = d_orec;
    G->occ_pos = d_opos;
    // ---- edges: the pair keys in ranges of their smaller end.  The histogram that plans the ranges counts the adjacent pairs, which
    // bound the edges; the one range of a build that fits has none and sizes the edge columns by its own count.
    std::vector<KeyRange> er;
    EdgeCols eu0 = {};
    if (sliced) {
      std::vector<uint64_t> ph;
      const uint32_t ushift = bin_shift(nv);
      if (int rc = slice_hist(ctx, PairBin{ d_cvid, d_casm, d_clist, m, ushift }, m, &ph)) return rc;
      uint64_t n_pairs = 0;
      for (uint64_t x : ph) n_pairs += x;
      slice_ranges(ph, cap, 0, ushift, &er, &oversize);
      if (int rc = edge_cols(ctx, false, n_pairs, &eu0)) return rc;
    } else {
      er.push_back({ 0, ~0ULL, m });
    }
    if (int rc = slice_bufs(ctx, max_range(er), true, &b)) return rc;
    graph_sample_peak(ctx);
    uint64_t ne = 0;
    for (const KeyRange& r : er) {
      const uint64_t ms = r.n;
      const uint32_t sb = (uint32_t)((ms + 255) / 256);
      const uint64_t* members = nullptr;
      if (sliced) {
        if (int rc = slice_select(ctx, PairIn{ d_cvid, d_casm, d_clist, m, r.lo, r.hi }, m, b.idx)) return rc;
        members = b.idx;
      }
      {
        ScopedTimer t(ctx, "graph_build");
        NTS_LAUNCH(k_g_gather_pairs, dim3(sb), dim3(256), 0, ctx->stream, members, ms, d_cvid, d_casm, d_clist, m, b.h);
        if (int rc = slice_sort(ctx, b, b.h, members, ms)) return rc;
        NTS_LAUNCH(k_g_edge_heads, dim3(sb), dim3(256), 0, ctx->stream, b.h2, ms, b.flag);
        if (int rc = slice_scan(ctx, b, ms)) return rc;
      }
      uint64_t ne_s = 0;
      if (int rc = flag_count(ctx, b.flag, b.scan, ms, &ne_s)) return rc;
      if (!sliced)
        if (int rc = edge_cols(ctx, false, ne_s, &eu0)) return rc;
      {
        ScopedTimer t(ctx, "graph_build");
        NTS_LAUNCH(k_g_edges, dim3(sb), dim3(256), 0, ctx->stream, b.h2, b.idx2, b.flag, b.scan, ms, d_cvid, eu0.u + ne, eu0.v + ne, eu0.w + ne,
                           eu0.first + ne);
      }
      ne += ne_s;
    }
    G->ne = ne;
    n_eslices = std::max<uint64_t>(er.size(), 1);
    EdgeCols eu;
    if (int rc = edge_cols(ctx, true, ne, &eu)) return rc;
    if (ne) {
      // ---- ntJoin's dict order, sorted in ranges of the source's rank
      NTS_WS(d_srank, unsigned long long*, "g_srank", nv * 8);
      const uint32_t eb = (uint32_t)((ne + 255) / 256);
      {
        ScopedTimer t(ctx, "graph_build");
        HIP_TRY(ctx, hipMemsetAsync(d_srank, 0xFF, nv * 8, ctx->stream));
        NTS_LAUNCH(k_g_src_rank, dim3(eb), dim3(256), 0, ctx->stream, eu0.u, eu0.first, ne, d_srank);
      }
      std::vector<KeyRange> orr;
      if (sliced) {
        std::vector<uint64_t> rh;
        const uint32_t rshift = bin_shift(m); // (a rank is the sequence number of a pair: below m)
        if (int rc = slice_hist(ctx, RankBin{ eu0.u, d_srank, rshift }, ne, &rh)) return rc;
        slice_ranges(rh, cap, 0, rshift, &orr, &oversize);
      } else {
        orr.push_back({ 0, ~0ULL, ne });
      }
      n_eslices = std::max<uint64_t>(n_eslices, orr.size());
      if (int rc = slice_bufs(ctx, max_range(orr), true, &b)) return rc;
      graph_sample_peak(ctx);
      uint64_t off = 0;
      for (const KeyRange& r : orr) {
        const uint64_t ns = r.n;
        const uint32_t sb = (uint32_t)((ns + 255) / 256);
        const uint64_t* members = nullptr;
        if (sliced) {
          if (int rc = slice_select(ctx, RankIn{ eu0.u, d_srank, r.lo, r.hi }, ne, b.idx)) return rc;
          members = b.idx;
        }
        ScopedTimer t(ctx, "graph_build");
        NTS_LAUNCH(k_g_gather_order, dim3(sb), dim3(256), 0, ctx->stream, members, ns, eu0.u, eu0.first, d_srank, b.h);
        if (int rc = slice_sort(ctx, b, b.h, members, ns)) return rc;
        NTS_LAUNCH(k_g_permute_edges, dim3(sb), dim3(256), 0, ctx->stream, b.idx2, ns, eu0.u, eu0.v, eu0.w, eu0.first, eu.u + off, eu.v + off,
                           eu.w + off, eu.first + off);
        off += ns;
      }
    }
    G->e_u = eu.u;
    G->e_v = eu.v;
    G->e_w = eu.w;
    G->e_first = eu.first;
  }
  HIP_TRY(ctx, hipGetLastError());
  graph_sample_peak(ctx);
  // a build that fits leaves its buffers cached for the next one on this context; the slice buffers and the survivor-sized
  // intermediates of a sliced one do not stay cached into the caller's table growth
  if (sliced) {
    for (const char* nm : SLICE_SCRATCH) ws_drop(ctx, nm);
    for (const char* nm : { "g_eu0", "g_ev0", "g_ew0", "g_ef0", "g_srank", "g_cvid", "g_casm", "g_clist" }) ws_drop(ctx, nm);
  }
  ctx->last_graph_v_slices = (uint32_t)n_vslices;
  ctx->last_graph_e_slices = (uint32_t)n_eslices;
  ctx->last_graph_oversize = oversize;
  return NTS_OK;
}

// slice scratch per item: the vertex pass's buffers (the pair and order passes use fewer of them) and the sort's temporary storage
uint64_t slice_bytes_per_item(nts_ctx* ctx, uint64_t n)
{
  size_t tmp = 0;
  (void)rocprim::radix_sort_pairs(nullptr, tmp, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr, n, 0, 64,
                                  ctx->stream);
  return 6 * 8 + 1 + (tmp + n - 1) / n;
}

// what the results of a build and the engine's tables may grow by, per input minimizer (vertices <= n / n_asm with a hash and n_asm
// occurrences each; survivors <= n with their columns, pairs, unordered and ordered edges; the engine's copies of both)
constexpr uint64_t GRAPH_RESULT_BYTES = 96;

// automatic budget: free device memory and the allocation cache's free bytes, less a margin, less what the build keeps n-sized
// besides the slices and what its results and the engine's tables may grow by
uint64_t graph_auto_budget(uint64_t n, bool hook)
{
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess) {
    (void)hipGetLastError();
    return ~0ULL; // (cannot tell: one range)
  }
  uint64_t cached = 0;
  {
    std::lock_guard<std::mutex> g(nts_mem::mu);
    cached = nts_mem::cached_bytes - nts_mem::cached_small;
  }
  const uint64_t margin = 1ull << 30;
  const uint64_t kept = n * (4 + 1 + (hook ? 16 : 0) + GRAPH_RESULT_BYTES);
  const uint64_t avail = (uint64_t)fr + cached;
  return avail > margin + kept ? avail - margin - kept : 1;
}

// The build proper: slices of budget / slice_bytes_per_item items; a build whose elements all fit one slice has one range per pass
// and plans nothing.  The same graph either way.
int graph_build_core(nts_ctx* ctx, uint32_t n_asm, uint64_t n, GraphDev* G, ListHook* hook)
{
  *G = GraphDev();
  G->n = n;
  ctx->last_graph_v_slices = ctx->last_graph_e_slices = 1;
  ctx->last_graph_oversize = 0;
  ctx->last_graph_peak = 0;
  if (n == 0) return NTS_OK;
  const uint64_t per_item = slice_bytes_per_item(ctx, n);
  const uint64_t budget = ctx->graph_budget ? ctx->graph_budget : graph_auto_budget(n, hook != nullptr);
  const uint64_t cap = budget / per_item;
  const int rc = graph_build_ranges(ctx, n_asm, n, G, hook, cap);
  if (rc == NTS_ENOMEM && n > cap)
    ctx->err += " (graph build in slices: budget " + std::to_string(budget) + " B, " + std::to_string(cap) + " minimizers per slice)";
  return rc;
}

// scratch buffers of the concatenation, sized for n elements
struct GraphIn
{
  uint64_t* h = nullptr;
  uint32_t* asm_id = nullptr;
  uint32_t* rec = nullptr;
  uint64_t* pos = nullptr;
  uint8_t* keep = nullptr;
  uint32_t* list = nullptr;
};

int graph_inputs(nts_ctx* ctx, uint64_t n, GraphIn* in)
{
  const uint64_t c = std::max<uint64_t>(n, 1);
  in->h = (uint64_t*)ws_get(ctx, "g_h", c * 8);
  in->asm_id = (uint32_t*)ws_get(ctx, "g_asm", c * 4);
  in->rec = (uint32_t*)ws_get(ctx, "g_rec", c * 4);
  in->pos = (uint64_t*)ws_get(ctx, "g_pos", c * 8);
  in->keep = (uint8_t*)ws_get(ctx, "g_keep", c);
  in->list = (uint32_t*)ws_get(ctx, "g_list", c * 4);
  return (in->h && in->asm_id && in->rec && in->pos && in->keep && in->list) ? NTS_OK : NTS_ENOMEM;
}

} // namespace

extern "C" int nts_graph_build(nts_ctx* ctx, uint32_t n_asm, const nts_mxlist* lists, nts_graph* out)
{
  if (!ctx || !out || n_asm == 0 || !lists) return fail(ctx, NTS_EINVAL, "nts_graph_build: bad arguments");
  memset(out, 0, sizeof(*out));
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ctx->graph_live0 = nts_mem::live.load();
  uint64_t n = 0;
  for (uint32_t a = 0; a < n_asm; ++a) {
    if (lists[a].n && (!lists[a].h1 || !lists[a].rec || !lists[a].pos)) return fail(ctx, NTS_EINVAL, "nts_graph_build: NULL list arrays");
    n += lists[a].n;
  }
  if (n >= 0xFFFFFFFFULL) return fail(ctx, NTS_ERANGE, "nts_graph_build: more than 2^32 minimizers");
  auto finish_empty = [&]() {
    out->v_hash = (uint64_t*)malloc(8);
    out->occ_rec = (uint32_t*)malloc(8);
    out->occ_pos = (uint64_t*)malloc(8);
    out->e_u = (uint32_t*)malloc(8);
    out->e_v = (uint32_t*)malloc(8);
    out->e_w = (uint32_t*)malloc(8);
    out->e_first = (uint64_t*)malloc(8);
    return NTS_OK;
  };
  if (n == 0) return finish_empty();
  GraphIn in;
  if (graph_inputs(ctx, n, &in) != NTS_OK) return NTS_ENOMEM;
  // assembly-major concatenation; the assembly ids are filled on the device, the keep mask is uploaded only where a list brings one
  uint64_t o = 0;
  for (uint32_t a = 0; a < n_asm; ++a) {
    const uint64_t m = lists[a].n;
    if (m) {
      HIP_TRY(ctx, hipMemcpyAsync(in.h + o, lists[a].h1, m * 8, hipMemcpyHostToDevice, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(in.rec + o, lists[a].rec, m * 4, hipMemcpyHostToDevice, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(in.pos + o, lists[a].pos, m * 8, hipMemcpyHostToDevice, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(in.list + o, lists[a].list_id ? lists[a].list_id : lists[a].rec, m * 4, hipMemcpyHostToDevice, ctx->stream));
      if (lists[a].keep)
        HIP_TRY(ctx, hipMemcpyAsync(in.keep + o, lists[a].keep, m, hipMemcpyHostToDevice, ctx->stream));
      else
        HIP_TRY(ctx, hipMemsetAsync(in.keep + o, 1, m, ctx->stream));
      HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)(in.asm_id + o), (int)a, m, ctx->stream));
    }
    o += m;
  }
  GraphDev G;
  if (int rc = graph_build_core(ctx, n_asm, n, &G, nullptr)) return rc;
  const uint64_t nv = G.nv, ne = G.ne;
  out->nv = nv;
  out->ne = ne;
  if (nv == 0) return finish_empty();
  out->v_hash = host_copy(ctx, G.v_hash, nv);
  out->occ_rec = host_copy(ctx, G.occ_rec, (uint64_t)n_asm * nv);
  out->occ_pos = host_copy(ctx, G.occ_pos, (uint64_t)n_asm * nv);
  out->e_u = host_copy(ctx, G.e_u, ne);
  out->e_v = host_copy(ctx, G.e_v, ne);
  out->e_w = host_copy(ctx, G.e_w, ne);
  out->e_first = host_copy(ctx, G.e_first, ne);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (!out->v_hash || !out->occ_rec || !out->occ_pos || !out->e_u || !out->e_v || !out->e_w || !out->e_first) {
    nts_graph_free(out);
    return fail(ctx, NTS_ENOMEM, "nts_graph_build: host allocation failed");
  }
  return NTS_OK;
}

namespace {
#include "nts_iv_links.inc"
#include "nts_iv_sites.inc"
#include "nts_iv_periods.inc"
#include "nts_iv_families.inc"
#include "nts_iv_anchors.inc"
#include "nts_edit.inc"
#include "nts_edit_fr_script.inc"
#include "nts_edit_script.inc"
#include "nts_edit_wide.inc"
#include "nts_edit_wide_script.inc"
#include "nts_edit_extend.inc"
#include "nts_edit_extend_script.inc"
#include "nts_cigar.inc"
} // namespace

extern "C" int nts_iv_links(nts_ctx* ctx, uint32_t n_lists, const nts_sample* const* lists, const uint64_t* n, uint32_t min_anchors, nts_iv_link** out,
                            uint64_t* n_out)
{
  if (!ctx || !out || !n_out || min_anchors == 0 || n_lists > IVL_MAX_LISTS || (n_lists && (!lists || !n)))
    return fail(ctx, NTS_EINVAL, "nts_iv_links: bad arguments (at most 64 lists, min_anchors >= 1)");
  for (uint32_t l = 0; l < n_lists; ++l)
    if (n[l] && !lists[l]) return fail(ctx, NTS_EINVAL, "nts_iv_links: NULL list");
  *out = nullptr;
  *n_out = 0;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return iv_links_run(ctx, n_lists, lists, n, min_anchors, out, n_out);
}

extern "C" int nts_iv_sites(nts_ctx* ctx, uint32_t n_lists, const nts_sample* const* lists, const uint64_t* n, const nts_sample* target,
                            uint64_t n_target, uint32_t step, uint32_t min_hits, nts_iv_site** out, uint64_t* n_out)
{
  if (!ctx || !out || !n_out || min_hits == 0 || n_lists > IVL_MAX_LISTS || (n_lists && (!lists || !n)) || (n_target && !target))
    return fail(ctx, NTS_EINVAL, "nts_iv_sites: bad arguments (at most 64 lists, min_hits >= 1)");
  for (uint32_t l = 0; l < n_lists; ++l)
    if (n[l] && !lists[l]) return fail(ctx, NTS_EINVAL, "nts_iv_sites: NULL list");
  *out = nullptr;
  *n_out = 0;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return iv_sites_run(ctx, n_lists, lists, n, target, n_target, step, min_hits, out, n_out);
}

extern "C" int nts_iv_periods(nts_ctx* ctx, const nts_sample* recs, uint64_t n, uint64_t n_iv, nts_iv_period* out)
{
  if (!ctx || (n && !recs) || (n_iv && !out)) return fail(ctx, NTS_EINVAL, "nts_iv_periods: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return iv_periods_run(ctx, recs, n, n_iv, out);
}

extern "C" int nts_iv_period_hashes(nts_ctx* ctx, const nts_sample* recs, uint64_t n, uint64_t n_iv, const uint32_t* period, nts_sample** out, uint64_t* n_out)
{
  if (!ctx || !out || !n_out || (n && !recs) || (n_iv && !period)) return fail(ctx, NTS_EINVAL, "nts_iv_period_hashes: bad arguments");
  *out = nullptr;
  *n_out = 0;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return iv_period_hashes_run(ctx, recs, n, n_iv, period, out, n_out);
}

extern "C" int nts_iv_families(nts_ctx* ctx, const nts_sample* pairs, uint64_t n, uint64_t n_arrays, uint32_t* family, uint64_t** hashes,
                               uint32_t** hash_family, uint64_t* n_hashes)
{
  if (!ctx || !hashes || !hash_family || !n_hashes || (n && !pairs) || (n_arrays && !family)) return fail(ctx, NTS_EINVAL, "nts_iv_families: bad arguments");
  *hashes = nullptr;
  *hash_family = nullptr;
  *n_hashes = 0;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return iv_families_run(ctx, pairs, n, n_arrays, family, hashes, hash_family, n_hashes);
}

extern "C" int nts_iv_family_sites(nts_ctx* ctx, const nts_sample* occ, uint64_t n_occ, const uint64_t* hashes, const uint32_t* hash_family,
                                   uint64_t n_hashes, uint32_t step, uint32_t min_hits, nts_iv_fsite** out, uint64_t* n_out)
{
  if (!ctx || !out || !n_out || min_hits == 0 || (n_occ && !occ) || (n_hashes && (!hashes || !hash_family)))
    return fail(ctx, NTS_EINVAL, "nts_iv_family_sites: bad arguments (min_hits >= 1)");
  *out = nullptr;
  *n_out = 0;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return iv_family_sites_run(ctx, occ, n_occ, hashes, hash_family, n_hashes, step, min_hits, out, n_out);
}

extern "C" int nts_iv_anchor_segments(nts_ctx* ctx, const nts_sample* recs_a, uint64_t n_a, const nts_sample* recs_b, uint64_t n_b, const uint32_t* mate,
                                      uint64_t n_iv_a, const uint32_t* len_b, const uint8_t* flip, uint32_t k, uint32_t band, uint32_t max_len,
                                      nts_iv_segment** segs, uint64_t* n_segs, uint32_t* anchors_per_iv)
{
  if (!ctx || !segs || !n_segs || (n_a && !recs_a) || (n_b && !recs_b) || (n_iv_a && (!mate || !len_b || !flip || !anchors_per_iv)) || k == 0 || band < 1 ||
      band > EDIT_MAX_BAND || max_len < 1 || max_len > EDIT_MAX_LEN)
    return fail(ctx, NTS_EINVAL, "nts_iv_anchor_segments: bad arguments (k >= 1, band 1..31, max_len 1..65535)");
  *segs = nullptr;
  *n_segs = 0;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return iv_anchor_segments_run(ctx, recs_a, n_a, recs_b, n_b, mate, n_iv_a, len_b, flip, k, band, max_len, segs, n_segs, anchors_per_iv);
}

extern "C" int nts_edit_segments(nts_ctx* ctx, const nts_genome* g_a, const nts_genome* g_b, const nts_interval* iv_a, const nts_interval* iv_b,
                                 const nts_iv_segment* segs, uint64_t n_segs, uint64_t n_iv_a, const uint8_t* flip, uint32_t band,
                                 nts_iv_identity* per_iv_out, uint32_t* dist_out)
{
  if (!ctx || !g_a || !g_b || (n_segs && !segs) || (n_iv_a && (!iv_a || !iv_b || !flip || !per_iv_out)) || band < 1 || band > EDIT_MAX_BAND)
    return fail(ctx, NTS_EINVAL, "nts_edit_segments: bad arguments (band 1..31)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return edit_segments_run(ctx, g_a, g_b, iv_a, iv_b, segs, n_segs, n_iv_a, flip, band, per_iv_out, dist_out);
}

extern "C" int nts_edit_script(nts_ctx* ctx, const nts_genome* g_a, const nts_genome* g_b, const nts_interval* iv_a, const nts_interval* iv_b,
                               const nts_iv_segment* segs, uint64_t n_segs, uint64_t n_iv_a, const uint8_t* flip, uint32_t band, const uint32_t* dist,
                               nts_edit_op** ops, uint64_t* n_ops, uint64_t* first)
{
  if (!ctx || !g_a || !g_b || !ops || !n_ops || (n_segs && (!segs || !dist)) || (n_iv_a && (!iv_a || !iv_b || !flip)) || band < 1 ||
      band > EDIT_MAX_BAND)
    return fail(ctx, NTS_EINVAL, "nts_edit_script: bad arguments (band 1..31)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return edit_script_run(ctx, g_a, g_b, iv_a, iv_b, segs, n_segs, n_iv_a, flip, band, dist, ops, n_ops, first);
}

extern "C" int nts_edit_wide(nts_ctx* ctx, const nts_genome* g_a, const nts_genome* g_b, const nts_interval* iv_a, const nts_interval* iv_b,
                             const nts_iv_segment* segs, uint64_t n_segs, uint64_t n_iv_a, const uint8_t* flip, uint32_t band, uint32_t max_edits,
                             const uint32_t* dist, nts_iv_identity* per_iv_out, uint32_t* dist_out)
{
  if (!ctx || !g_a || !g_b || (n_segs && (!segs || !dist)) || (n_iv_a && (!iv_a || !iv_b || !flip || !per_iv_out)) || band < 1 || band > EDIT_MAX_BAND ||
      max_edits < 2 * band + 1 || max_edits > WIDE_MAX_EDITS)
    return fail(ctx, NTS_EINVAL, "nts_edit_wide: bad arguments (band 1..31, max_edits 2 band + 1..1023)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return edit_wide_run(ctx, g_a, g_b, iv_a, iv_b, segs, n_segs, n_iv_a, flip, band, max_edits, dist, per_iv_out, dist_out);
}

extern "C" int nts_edit_wide_script(nts_ctx* ctx, const nts_genome* g_a, const nts_genome* g_b, const nts_interval* iv_a, const nts_interval* iv_b,
                                    const nts_iv_segment* segs, uint64_t n_segs, uint64_t n_iv_a, const uint8_t* flip, uint32_t band, uint32_t max_edits,
                                    const uint32_t* dist, uint64_t table_budget, nts_edit_op** ops, uint64_t* n_ops, uint64_t* first)
{
  if (!ctx || !g_a || !g_b || !ops || !n_ops || (n_segs && (!segs || !dist)) || (n_iv_a && (!iv_a || !iv_b || !flip)) || band < 1 || band > EDIT_MAX_BAND ||
      max_edits < 2 * band + 1 || max_edits > WIDE_MAX_EDITS)
    return fail(ctx, NTS_EINVAL, "nts_edit_wide_script: bad arguments (band 1..31, max_edits 2 band + 1..1023)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return edit_wide_script_run(ctx, g_a, g_b, iv_a, iv_b, segs, n_segs, n_iv_a, flip, band, max_edits, dist, table_budget, ops, n_ops, first);
}

extern "C" int nts_edit_wide_script_last_plan(nts_ctx* ctx, uint64_t* members, uint64_t* table_bytes, uint64_t* batches)
{
  if (!ctx) return NTS_EINVAL;
  if (members) *members = ctx->last_wscript_members;
  if (table_bytes) *table_bytes = ctx->last_wscript_table_bytes;
  if (batches) *batches = ctx->last_wscript_batches;
  return NTS_OK;
}

extern "C" int nts_edit_extend(nts_ctx* ctx, const nts_genome* g_a, const nts_genome* g_b, const nts_extend_task* tasks, uint64_t n_tasks,
                               uint32_t penalty, uint32_t max_edits, nts_extend_result* out)
{
  if (!ctx || !g_a || !g_b || (n_tasks && (!tasks || !out)) || penalty < EXTEND_MIN_PENALTY || penalty > EXTEND_MAX_PENALTY || max_edits < 1 ||
      max_edits > EXTEND_MAX_EDITS)
    return fail(ctx, NTS_EINVAL, "nts_edit_extend: bad arguments (penalty 3..255, max_edits 1..1023)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return edit_extend_run(ctx, g_a, g_b, tasks, n_tasks, penalty, max_edits, out);
}

extern "C" int nts_edit_extend_script(nts_ctx* ctx, const nts_genome* g_a, const nts_genome* g_b, const nts_extend_task* tasks, uint64_t n_tasks,
                                      const nts_extend_result* results, uint64_t table_budget, nts_edit_op** ops, uint64_t* n_ops, uint64_t* first)
{
  if (!ctx || !g_a || !g_b || !ops || !n_ops || (n_tasks && (!tasks || !results))) return fail(ctx, NTS_EINVAL, "nts_edit_extend_script: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return edit_extend_script_run(ctx, g_a, g_b, tasks, n_tasks, results, table_budget, ops, n_ops, first);
}

extern "C" int nts_edit_extend_script_last_plan(nts_ctx* ctx, uint64_t* members, uint64_t* table_bytes, uint64_t* batches)
{
  if (!ctx) return NTS_EINVAL;
  if (members) *members = ctx->last_escript_members;
  if (table_bytes) *table_bytes = ctx->last_escript_table_bytes;
  if (batches) *batches = ctx->last_escript_batches;
  return NTS_OK;
}

extern "C" int nts_cigar_build(nts_ctx* ctx, const nts_cig_piece* pieces, uint64_t n_pieces, uint64_t n_chains, const nts_edit_op* ops,
                               const uint64_t* first, uint64_t** cigar, uint64_t* n_cigar, nts_cig_chain* chains)
{
  if (!ctx || !cigar || !n_cigar || !first || (n_pieces && !pieces) || (n_chains && !chains)) return fail(ctx, NTS_EINVAL, "nts_cigar_build: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cigar_build_run(ctx, pieces, n_pieces, n_chains, ops, first, cigar, n_cigar, chains);
}

extern "C" int nts_cigar_text(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains, const nts_genome* a,
                              const nts_genome* b, const nts_cig_span* spans, uint8_t** cg, uint64_t* cg_first, uint8_t** cs, uint64_t* cs_first)
{
  if (!ctx) return NTS_EINVAL;
  if (n_cigar > 0xFFFFFFFFull || n_chains > 0xFFFFFFFFull) // (before any array is read)
    return fail(ctx, NTS_ERANGE, "nts_cigar_text: 2^32 entries or chains or more");
  if ((n_cigar && !cigar) || (n_chains && !chains) || !cg || !cg_first || (spans && (!cs || !cs_first))) return fail(ctx, NTS_EINVAL, "nts_cigar_text: bad arguments");
  if (spans ? !a || !b : a || b) return fail(ctx, NTS_EINVAL, "nts_cigar_text: spans go with both genomes, no spans with none");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cigar_text_run(ctx, cigar, n_cigar, chains, n_chains, a, b, spans, cg, cg_first, cs, cs_first);
}

extern "C" int nts_cigar_lift(nts_ctx* ctx,const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains,
                              const nts_lift_query* queries, uint64_t n_queries, nts_lift_hit* hits)
{
  if (!ctx) return NTS_EINVAL;
  if (n_cigar > 0xFFFFFFFFull || n_chains > 0xFFFFFFFFull || n_queries > 0xFFFFFFFFull) // (before any array is read)
    return fail(ctx, NTS_ERANGE, "nts_cigar_lift: 2^32 entries, chains or queries or more");
  if ((n_cigar && !cigar) || (n_chains && !chains) || (n_queries && (!queries || !hits))) return fail(ctx, NTS_EINVAL, "nts_cigar_lift: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cigar_lift_run(ctx, cigar, n_cigar, chains, n_chains, queries, n_queries, hits);
}

extern "C" int nts_cigar_lift_stats(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains,
                                    const nts_lift_range* ranges, uint64_t n_ranges, nts_lift_stats* stats)
{
  if (!ctx) return NTS_EINVAL;
  if (n_cigar > 0xFFFFFFFFull || n_chains > 0xFFFFFFFFull || n_ranges > 0xFFFFFFFFull) // (before any array is read)
    return fail(ctx, NTS_ERANGE, "nts_cigar_lift_stats: 2^32 entries, chains or ranges or more");
  if ((n_cigar && !cigar) || (n_chains && !chains) || (n_ranges && (!ranges || !stats))) return fail(ctx, NTS_EINVAL, "nts_cigar_lift_stats: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cigar_lift_stats_run(ctx, cigar, n_cigar, chains, n_chains, ranges, n_ranges, stats);
}

extern "C" int nts_cigar_lift_pairs(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains,
                                    const nts_lift_link* links, uint64_t n_links, const uint64_t* pair_first, uint64_t n_pairs,
                                    const nts_pair_range* ranges, uint64_t n_ranges, nts_pair_stats* stats)
{
  if (!ctx) return NTS_EINVAL;
  if (n_cigar > 0xFFFFFFFFull || n_chains > 0xFFFFFFFFull) // (before any array is read)
    return fail(ctx, NTS_ERANGE, "nts_cigar_lift_pairs: 2^32 entries or chains or more");
  if (n_links > 0xFFFFFFFFull || n_pairs > 0xFFFFFFFFull || n_ranges > 0xFFFFFFFFull)
    return fail(ctx, NTS_ERANGE, "nts_cigar_lift_pairs: 2^32 links, pairs or ranges or more");
  if ((n_cigar && !cigar) || (n_chains && !chains) || (n_links && !links) || !pair_first || (n_ranges && (!ranges || !stats)))
    return fail(ctx, NTS_EINVAL, "nts_cigar_lift_pairs: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cigar_lift_pairs_run(ctx, cigar, n_cigar, chains, n_chains, links, n_links, pair_first, n_pairs, ranges, n_ranges, stats);
}

extern "C" int nts_cigar_chain_blocks(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains,
                                      const nts_lift_link* links, uint64_t n_links, const uint64_t* pair_first, uint64_t n_pairs, nts_chain_pair* pairs,
                                      nts_chain_block** blocks, uint64_t* n_blocks, uint8_t** text, uint64_t* text_first)
{
  if (!ctx) return NTS_EINVAL;
  if (n_cigar > 0xFFFFFFFFull || n_chains > 0xFFFFFFFFull) // (before any array is read)
    return fail(ctx, NTS_ERANGE, "nts_cigar_chain_blocks: 2^32 entries or chains or more");
  if (n_links > 0xFFFFFFFFull || n_pairs > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_cigar_chain_blocks: 2^32 links or pairs or more");
  if ((n_cigar && !cigar) || (n_chains && !chains) || (n_links && !links) || !pair_first || (n_pairs && !pairs) || !blocks || !n_blocks ||
      (text == nullptr) != (text_first == nullptr))
    return fail(ctx, NTS_EINVAL, "nts_cigar_chain_blocks: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cigar_chain_blocks_run(ctx, cigar, n_cigar, chains, n_chains, links, n_links, pair_first, n_pairs, pairs, blocks, n_blocks, text, text_first);
}

extern "C" int nts_cigar_rows(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains, const nts_genome* a,
                              const nts_genome* b, const nts_cig_span* spans, uint8_t** row_a, uint8_t** row_b, uint64_t* row_first)
{
  if (!ctx) return NTS_EINVAL;
  if (n_cigar > 0xFFFFFFFFull || n_chains > 0xFFFFFFFFull) // (before any array is read)
    return fail(ctx, NTS_ERANGE, "nts_cigar_rows: 2^32 entries or chains or more");
  if ((n_cigar && !cigar) || (n_chains && !chains) || !row_a || !row_b || !row_first) return fail(ctx, NTS_EINVAL, "nts_cigar_rows: bad arguments");
  if (!a || !b || !spans) return fail(ctx, NTS_EINVAL, "nts_cigar_rows: the rows need spans and both genomes");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cigar_rows_run<false>(ctx, cigar, n_cigar, chains, n_chains, a, b, spans, row_a, row_b, row_first);
}

extern "C" int nts_cigar_rows_padded(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains,
                                     const nts_genome* a, const nts_genome* b, const nts_cig_span* spans, uint8_t** row_a, uint8_t** row_b,
                                     uint64_t* row_first)
{
  if (!ctx) return NTS_EINVAL;
  if (n_cigar > 0xFFFFFFFFull || n_chains > 0xFFFFFFFFull) // (before any array is read)
    return fail(ctx, NTS_ERANGE, "nts_cigar_rows_padded: 2^32 entries or chains or more");
  if ((n_cigar && !cigar) || (n_chains && !chains) || !row_a || !row_b || !row_first)
    return fail(ctx, NTS_EINVAL, "nts_cigar_rows_padded: bad arguments");
  if (!a || !b || !spans) return fail(ctx, NTS_EINVAL, "nts_cigar_rows_padded: the rows need spans and both genomes");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cigar_rows_run<true>(ctx, cigar, n_cigar, chains, n_chains, a, b, spans, row_a, row_b, row_first);
}

extern "C" int nts_cigar_pad(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains,
                             const nts_cig_pad_at* at, uint64_t n_groups, uint64_t** padded, uint64_t* pad_first, uint64_t* site_first,
                             uint64_t** site_pos, uint64_t** site_w)
{
  if (!ctx) return NTS_EINVAL;
  if (n_cigar > 0xFFFFFFFFull || n_chains > 0xFFFFFFFFull || n_groups > 0xFFFFFFFFull) // (before any array is read)
    return fail(ctx, NTS_ERANGE, "nts_cigar_pad: 2^32 entries, chains or groups or more");
  if ((n_cigar && !cigar) || (n_chains && (!chains || !at)) || !padded || !pad_first || !site_first || !site_pos || !site_w)
    return fail(ctx, NTS_EINVAL, "nts_cigar_pad: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cigar_pad_run(ctx, cigar, n_cigar, chains, n_chains, at, n_groups, padded, pad_first, site_first, site_pos, site_w);
}

extern "C" int nts_cigar_depth(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains,
                               const nts_cig_pad_at* at, uint64_t n_groups, nts_cig_depth_seg** segs, uint64_t* seg_first)
{
  if (!ctx) return NTS_EINVAL;
  if (n_cigar > 0xFFFFFFFFull || n_chains > 0xFFFFFFFFull || n_groups > 0xFFFFFFFFull) // (before any array is read)
    return fail(ctx, NTS_ERANGE, "nts_cigar_depth: 2^32 entries, chains or groups or more");
  if ((n_cigar && !cigar) || (n_chains && (!chains || !at)) || !segs || !seg_first) return fail(ctx, NTS_EINVAL, "nts_cigar_depth: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cigar_depth_run(ctx, cigar, n_cigar, chains, n_chains, at, n_groups, segs, seg_first);
}

extern "C" int nts_cigar_var_bases(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains,
                                   const nts_genome* a, const nts_genome* b, const nts_cig_span* spans, uint8_t** ref, uint64_t* ref_first, uint8_t** alt,
                                   uint64_t* alt_first)
{
  if (!ctx) return NTS_EINVAL;
  if (n_cigar > 0xFFFFFFFFull || n_chains > 0xFFFFFFFFull) // (before any array is read)
    return fail(ctx, NTS_ERANGE, "nts_cigar_var_bases: 2^32 entries or chains or more");
  if ((n_cigar && !cigar) || (n_chains && !chains) || !ref || !ref_first || !alt || !alt_first)
    return fail(ctx, NTS_EINVAL, "nts_cigar_var_bases: bad arguments");
  if (!a || !b || !spans) return fail(ctx, NTS_EINVAL, "nts_cigar_var_bases: the bytes need spans and both genomes");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cigar_var_bases_run(ctx, cigar, n_cigar, chains, n_chains, a, b, spans, ref, ref_first, alt, alt_first);
}

extern "C" int nts_cigar_alleles(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains,
                                 const nts_cig_pad_at* at, uint64_t n_groups, const uint8_t* alt, uint64_t n_alt, nts_cig_allele** alleles,
                                 uint64_t* allele_first, uint32_t** carriers, uint64_t* n_carriers)
{
  if (!ctx) return NTS_EINVAL;
  if (n_cigar > 0xFFFFFFFFull || n_chains > 0xFFFFFFFFull || n_groups > 0xFFFFFFFFull) // (before any array is read)
    return fail(ctx, NTS_ERANGE, "nts_cigar_alleles: 2^32 entries, chains or groups or more");
  if ((n_cigar && !cigar) || (n_chains && (!chains || !at)) || (n_alt && !alt) || !alleles || !allele_first || !carriers || !n_carriers)
    return fail(ctx, NTS_EINVAL, "nts_cigar_alleles: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cigar_alleles_run(ctx, cigar, n_cigar, chains, n_chains, at, n_groups, alt, n_alt, alleles, allele_first, carriers, n_carriers);
}

extern "C" int nts_cigar_profile(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains,
                                 const nts_cig_pad_at* at, uint64_t n_groups, const uint8_t* ref, uint64_t n_ref, const uint8_t* alt, uint64_t n_alt,
                                 nts_cig_profile_col** cols, uint64_t* col_first)
{
  if (!ctx) return NTS_EINVAL;
  if (n_cigar > 0xFFFFFFFFull || n_chains > 0xFFFFFFFFull || n_groups > 0xFFFFFFFFull) // (before any array is read)
    return fail(ctx, NTS_ERANGE, "nts_cigar_profile: 2^32 entries, chains or groups or more");
  if ((n_cigar && !cigar) || (n_chains && (!chains || !at)) || (n_ref && !ref) || (n_alt && !alt) || !cols || !col_first)
    return fail(ctx, NTS_EINVAL, "nts_cigar_profile: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return cigar_profile_run(ctx, cigar, n_cigar, chains, n_chains, at, n_groups, ref, n_ref, alt, n_alt, cols, col_first);
}

extern "C" int nts_graph_budget(nts_ctx* ctx, uint64_t bytes)
{
  if (!ctx) return NTS_EINVAL;
  ctx->graph_budget = bytes;
  return NTS_OK;
}

extern "C" int nts_graph_last_plan(nts_ctx* ctx, uint32_t* v_slices, uint32_t* e_slices, uint64_t* scratch_peak_bytes, uint32_t* oversize_slices)
{
  if (!ctx) return NTS_EINVAL;
  if (v_slices) *v_slices = ctx->last_graph_v_slices;
  if (e_slices) *e_slices = ctx->last_graph_e_slices;
  if (scratch_peak_bytes) *scratch_peak_bytes = ctx->last_graph_peak;
  if (oversize_slices) *oversize_slices = ctx->last_graph_oversize;
  return NTS_OK;
}

// greedy: bins go into the running slice while its items times bytes_per_elem stay within the budget; a bin that alone exceeds it
// is a slice of its own
extern "C" int nts_graph_plan_slices(const uint64_t* hist, uint32_t n_bins, uint64_t bytes_per_elem, uint64_t budget, uint32_t* cuts, uint32_t* n_slices)
{
  if (!hist || !cuts || !n_slices || n_bins == 0 || bytes_per_elem == 0 || budget == 0) return NTS_EINVAL;
  const uint64_t cap = budget / bytes_per_elem;
  uint32_t s = 0;
  uint64_t acc = 0;
  cuts[0] = 0;
  for (uint32_t b = 0; b < n_bins; ++b) {
    if (acc > 0 && hist[b] > 0 && acc + hist[b] > cap) {
      cuts[++s] = b;
      acc = 0;
    }
    acc += hist[b];
  }
  cuts[++s] = n_bins;
  *n_slices = s;
  return NTS_OK;
}

#include "nts_dgraph.inc"

extern "C" void nts_graph_free(nts_graph* g)
{
  if (!g) return;
  free(g->v_hash);
  free(g->occ_rec);
  free(g->occ_pos);
  free(g->e_u);
  free(g->e_v);
  free(g->e_w);
  free(g->e_first);
  memset(g, 0, sizeof(*g));
}

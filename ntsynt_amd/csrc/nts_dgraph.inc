// nts_dgraph.inc -- the minimizer graph of a run, resident in HBM across rounds (rows C1-C9, C11, C12-erosion), included by
// ntsynt_hip.hip after the graph build core.
//
// The reference keeps the graph in igraph + Python dicts (bin/ntsynt_synteny.py with ntJoin's helpers) and walks it
// vertex by vertex.  Here the state is a set of flat device arrays and every rule is a pass over all vertices / edges /
// path positions at once:
//
//   nts_engine_add      build_graph(list_mxs, weights, graph=self.graph, black_list=terminals)   S:483, S:612, with the
//                       refinement round's position filters (S:256-280: internal hashes, block interiors, list cuts)
//   nts_engine_bubbles  the sub-graph around bubble candidates for run_graph_simplification (S:566-590); the rule itself is
//                       order dependent and rare, it runs on the host over this small table (ntsynt_amd/synteny_device.py)
//   nts_engine_apply    its result: vertices to delete, edge weights to promote
//   nts_engine_filter   filter_graph_global / filter_graph_global_flag_overlaps (S:292-303, S:491, S:617)
//   nts_engine_erode    refine_graph + erode_edges (S:305-362)
//   nts_engine_blocks   find_paths (ntJoin; S:492, S:620) as list ranking by pointer jumping over the degree <= 2 graph,
//                       then find_synteny_blocks / determine_orientations / check_for_indels / filter_synteny_blocks
//                       (S:66-106, synteny_block.py:48-70, S:364-426) as segment passes over the path order; only the
//                       block table (a few numbers per block) returns to the host.
// S:<line> = bin/ntsynt_synteny.py of the reference.
#include <rocprim/rocprim.hpp>

struct nts_engine
{
  uint32_t G = 0, ref = 0;
  uint64_t nv = 0, ne = 0, cap_v = 0, cap_e = 0;
  uint64_t* v_hash = nullptr;
  uint8_t* v_alive = nullptr;
  uint32_t* v_rec = nullptr; // [G][cap_v]
  uint64_t* v_pos = nullptr; // [G][cap_v]
  uint8_t* internal = nullptr;
  uint8_t* terminal = nullptr;
  uint32_t *e_u = nullptr, *e_v = nullptr, *e_w = nullptr;
  uint8_t* e_alive = nullptr;
  uint32_t *fl_u = nullptr, *fl_v = nullptr; // light edges flagged by the last filter
  uint64_t n_flag = 0, cap_flag = 0;
  // the path order of the last nts_engine_blocks call lives in the context's scratch
  uint64_t n_path_verts = 0, n_paths = 0;
};

namespace {

constexpr uint32_t E_NONE = 0xFFFFFFFFu;
constexpr uint32_t E_BAD = 0xFFFFFFFEu;
constexpr uint64_t IV_OFF = (uint64_t)1 << 40; // composite interval key: record * 2^40 + position (ntsynt_amd/synteny.py)

#define E_GRID(n) dim3((uint32_t)(((n) + 255) / 256)), dim3(256), 0, ctx->stream

template <typename T>
int e_grow(nts_ctx* ctx, T** p, uint64_t old_n, uint64_t new_cap)
{
  T* q = nullptr;
  if (dev_malloc((void**)&q, std::max<uint64_t>(new_cap, 1) * sizeof(T)) != hipSuccess) return fail(ctx, NTS_ENOMEM, "engine: hipMalloc");
  if (*p && old_n) hipMemcpyAsync(q, *p, old_n * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream);
  if (*p) {
    hipStreamSynchronize(ctx->stream);
    dev_free(*p);
  }
  *p = q;
  return NTS_OK;
}

int e_reserve_vertices(nts_ctx* ctx, nts_engine* E, uint64_t need)
{
  if (need <= E->cap_v) return NTS_OK;
  const uint64_t cap = need + need / 4 + 1024;
  if (int rc = e_grow(ctx, &E->v_hash, E->nv, cap)) return rc;
  if (int rc = e_grow(ctx, &E->v_alive, E->nv, cap)) return rc;
  if (int rc = e_grow(ctx, &E->internal, E->nv, cap)) return rc;
  if (int rc = e_grow(ctx, &E->terminal, E->nv, cap)) return rc;
  // the per-assembly rows change their stride
  uint32_t* nr = nullptr;
  uint64_t* np = nullptr;
  if (dev_malloc((void**)&nr, (uint64_t)E->G * cap * 4) != hipSuccess || dev_malloc((void**)&np, (uint64_t)E->G * cap * 8) != hipSuccess)
    return fail(ctx, NTS_ENOMEM, "engine: hipMalloc vertex tables");
  for (uint32_t a = 0; a < E->G && E->nv; ++a) {
    hipMemcpyAsync(nr + (uint64_t)a * cap, E->v_rec + (uint64_t)a * E->cap_v, E->nv * 4, hipMemcpyDeviceToDevice, ctx->stream);
    hipMemcpyAsync(np + (uint64_t)a * cap, E->v_pos + (uint64_t)a * E->cap_v, E->nv * 8, hipMemcpyDeviceToDevice, ctx->stream);
  }
  hipStreamSynchronize(ctx->stream);
  dev_free(E->v_rec);
  dev_free(E->v_pos);
  E->v_rec = nr;
  E->v_pos = np;
  E->cap_v = cap;
  return NTS_OK;
}

int e_reserve_edges(nts_ctx* ctx, nts_engine* E, uint64_t need)
{
  if (need <= E->cap_e) return NTS_OK;
  const uint64_t cap = need + need / 4 + 1024;
  if (int rc = e_grow(ctx, &E->e_u, E->ne, cap)) return rc;
  if (int rc = e_grow(ctx, &E->e_v, E->ne, cap)) return rc;
  if (int rc = e_grow(ctx, &E->e_w, E->ne, cap)) return rc;
  if (int rc = e_grow(ctx, &E->e_alive, E->ne, cap)) return rc;
  E->cap_e = cap;
  return NTS_OK;
}

template <typename T>
int e_fetch(nts_ctx* ctx, const T* d, T* h, uint64_t n = 1)
{
  HIP_TRY(ctx, hipMemcpyAsync(h, d, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return NTS_OK;
}

// ---- small device helpers ------------------------------------------------------------------------------------------
// first index i in [0, n) with a[i] >= x (n if none)
__device__ __forceinline__ uint64_t lower_bound_u64(const uint64_t* __restrict__ a, uint64_t n, uint64_t x)
{
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (a[mid] < x)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// "does [s0, e0) of record r reach into a block interior of r?" -- ntsynt_amd/synteny.py `overlaps` (S:194-203, S:267-275):
// intervals as composite keys sorted by start, cm = running maximum of the composite ends
__device__ __forceinline__ bool iv_overlaps(const uint64_t* __restrict__ cs, const uint64_t* __restrict__ cm, uint64_t n_iv, uint64_t r,
                                            uint64_t s0, uint64_t e0)
{
  if (n_iv == 0 || !(e0 > s0)) return false;
  const uint64_t base = r * IV_OFF;
  const uint64_t i = lower_bound_u64(cs, n_iv, base + e0);
  if (i == 0) return false;
  const uint64_t j = i - 1;
  return cs[j] >= base && cm[j] > base + s0;
}

// str(a) > str(b) for the decimal strings of two unsigned numbers (the reference orders a flagged pair by vertex NAME, S:351)
__device__ __forceinline__ bool dec_str_greater(uint64_t a, uint64_t b)
{
  auto digits = [](uint64_t x) {
    int n = 1;
    while (x >= 10) {
      x /= 10;
      ++n;
    }
    return n;
  };
  const int la = digits(a), lb = digits(b);
  if (la == lb) return a > b;
  uint64_t pa = a, pb = b;
  for (int i = la; i > lb; --i) pa /= 10; // the first min(la, lb) digits of each
  for (int i = lb; i > la; --i) pb /= 10;
  if (pa != pb) return pa > pb;
  return la > lb; // one is a prefix of the other: the longer string is the greater
}

// ---- kernels: add -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_e_live_flag(const uint8_t* __restrict__ alive, uint64_t nv, uint64_t* __restrict__ flag)
{
  const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v < nv) flag[v] = alive[v] ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_e_live_pairs(const uint8_t* __restrict__ alive, const uint64_t* __restrict__ where,
                                                      const uint64_t* __restrict__ v_hash, uint64_t nv, uint64_t* __restrict__ hs,
                                                      uint32_t* __restrict__ hid)
{
  const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv || !alive[v]) return;
  hs[where[v]] = v_hash[v];
  hid[where[v]] = (uint32_t)v;
}

// refinement round, per new minimizer: drop it if its hash is an internal minimizer of a block (S:274 `mx not in black_list`
// side of filter_minimizers_synteny_blocks) or its position lies in a block interior (S:274-275)
__global__ __launch_bounds__(256) void k_e_keep(const uint64_t* __restrict__ h, const uint32_t* __restrict__ asm_of,
                                                const uint32_t* __restrict__ rec, const uint64_t* __restrict__ pos, uint64_t n,
                                                const uint64_t* __restrict__ hs, const uint32_t* __restrict__ hid, uint64_t nl,
                                                const uint8_t* __restrict__ internal, const uint64_t* __restrict__ cs,
                                                const uint64_t* __restrict__ cm, const uint64_t* __restrict__ iv_off, uint8_t* __restrict__ keep)
{
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  bool k = true;
  const uint64_t x = h[e];
  const uint64_t p = lower_bound_u64(hs, nl, x);
  if (p < nl && hs[p] == x && internal[hid[p]]) k = false;
  const uint32_t a = asm_of[e];
  const uint64_t o = iv_off[a], m = iv_off[a + 1] - o;
  if (k && iv_overlaps(cs + o, cm + o, m, rec[e], pos[e], pos[e] + 1)) k = false;
  keep[e] = k ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_e_lastvalid_in(const uint8_t* __restrict__ valid, uint64_t n, uint64_t* __restrict__ out)
{
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) out[e] = valid[e] ? e + 1 : 0;
}

// a new list starts at every record change and wherever the span from the previous kept minimizer of the record to this
// kept minimizer crosses a block interior (S:267-273)
__global__ __launch_bounds__(256) void k_e_newlist(const uint8_t* __restrict__ valid, const uint64_t* __restrict__ lastvalid,
                                                   const uint32_t* __restrict__ asm_of, const uint32_t* __restrict__ rec,
                                                   const uint64_t* __restrict__ pos, uint64_t n, const uint64_t* __restrict__ cs,
                                                   const uint64_t* __restrict__ cm, const uint64_t* __restrict__ iv_off, uint64_t* __restrict__ flag)
{
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  bool nl = e == 0 || asm_of[e] != asm_of[e - 1] || rec[e] != rec[e - 1];
  if (!nl && valid[e]) {
    const uint64_t lv = lastvalid[e - 1]; // 1 + index of the last valid element before e, 0 = none
    if (lv) {
      const uint64_t q = lv - 1;
      const uint32_t a = asm_of[e];
      if (asm_of[q] == a && rec[q] == rec[e]) {
        const uint64_t o = iv_off[a], m = iv_off[a + 1] - o;
        if (iv_overlaps(cs + o, cm + o, m, rec[e], pos[q], pos[e])) nl = true;
      }
    }
  }
  flag[e] = nl ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_e_listid(const uint64_t* __restrict__ scan_incl, uint64_t n, uint32_t* __restrict__ list)
{
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) list[e] = (uint32_t)scan_incl[e];
}

// local vertex -> the live vertex carrying its hash, or new
__global__ __launch_bounds__(256) void k_e_lookup(const uint64_t* __restrict__ lh, uint64_t lnv, const uint64_t* __restrict__ hs,
                                                  const uint32_t* __restrict__ hid, uint64_t nl, uint32_t* __restrict__ l2g,
                                                  uint64_t* __restrict__ is_new)
{
  const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= lnv) return;
  const uint64_t x = lh[v];
  const uint64_t p = lower_bound_u64(hs, nl, x);
  const bool hit = p < nl && hs[p] == x;
  l2g[v] = hit ? hid[p] : E_NONE;
  is_new[v] = hit ? 0 : 1;
}

__global__ __launch_bounds__(256) void k_e_put_vertices(const uint64_t* __restrict__ lh, const uint32_t* __restrict__ occ_rec,
                                                        const uint64_t* __restrict__ occ_pos, uint64_t lnv, uint32_t G,
                                                        uint32_t* __restrict__ l2g, const uint64_t* __restrict__ new_rank, uint64_t nv0,
                                                        uint64_t cap_v, uint64_t* __restrict__ v_hash, uint8_t* __restrict__ v_alive,
                                                        uint8_t* __restrict__ internal, uint8_t* __restrict__ terminal,
                                                        uint32_t* __restrict__ v_rec, uint64_t* __restrict__ v_pos)
{
  const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= lnv) return;
  uint32_t g = l2g[v];
  if (g == E_NONE) {
    g = (uint32_t)(nv0 + new_rank[v]);
    l2g[v] = g;
    v_hash[g] = lh[v];
    v_alive[g] = 1;
    internal[g] = 0;
    terminal[g] = 0;
  }
  // S:282-290: positions of every hash that survived the filters are overwritten
  for (uint32_t a = 0; a < G; ++a) {
    v_rec[(uint64_t)a * cap_v + g] = occ_rec[(uint64_t)a * lnv + v];
    v_pos[(uint64_t)a * cap_v + g] = occ_pos[(uint64_t)a * lnv + v];
  }
}

// new edges in global numbering; those between two vertices that existed before this build may already exist
__global__ __launch_bounds__(256) void k_e_map_edges(const uint32_t* __restrict__ lu, const uint32_t* __restrict__ lv, uint64_t lne,
                                                     const uint32_t* __restrict__ l2g, uint64_t nv0, uint32_t* __restrict__ gu,
                                                     uint32_t* __restrict__ gv, uint64_t* __restrict__ old_old)
{
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= lne) return;
  const uint32_t u = l2g[lu[e]], v = l2g[lv[e]];
  gu[e] = u;
  gv[e] = v;
  old_old[e] = (u < nv0 && v < nv0) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_e_take_flagged(const uint64_t* __restrict__ flag, const uint64_t* __restrict__ where, uint64_t n,
                                                        const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                        const uint32_t* __restrict__ c, uint32_t* __restrict__ o_idx,
                                                        uint32_t* __restrict__ o_a, uint32_t* __restrict__ o_b, uint32_t* __restrict__ o_c)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !flag[i]) return;
  const uint64_t o = where[i];
  o_idx[o] = (uint32_t)i;
  o_a[o] = a[i];
  o_b[o] = b[i];
  if (c) o_c[o] = c[i];
}

// (smaller end << 32) | larger end of every pair
__global__ __launch_bounds__(256) void k_e_pair_keys(const uint32_t* __restrict__ u, const uint32_t* __restrict__ v, uint64_t n, uint64_t* __restrict__ key)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t a = min(u[i], v[i]), b = max(u[i], v[i]);
  key[i] = ((uint64_t)a << 32) | b;
}

// new edges against the sorted keys of the live edges at their ends: hit[i] = 1 and edge[i] = the (first, i.e. oldest) live edge of the same pair
__global__ __launch_bounds__(256) void k_e_join_pairs(const uint32_t* __restrict__ qu, const uint32_t* __restrict__ qv, uint64_t nq,
                                                      const uint64_t* __restrict__ key, const uint32_t* __restrict__ key_edge, uint64_t nk,
                                                      uint64_t* __restrict__ hit, uint32_t* __restrict__ edge)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  const uint32_t a = min(qu[i], qv[i]), b = max(qu[i], qv[i]);
  const uint64_t want = ((uint64_t)a << 32) | b;
  uint64_t lo = 0, hi = nk;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (key[mid] < want)
      lo = mid + 1;
    else
      hi = mid;
  }
  const bool found = lo < nk && key[lo] == want;
  hit[i] = found ? 1ull : 0ull;
  edge[i] = found ? key_edge[lo] : 0u;
}

__global__ __launch_bounds__(256) void k_e_touch(const uint32_t* __restrict__ u, const uint32_t* __restrict__ v, uint64_t n, uint8_t* __restrict__ touched)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  touched[u[i]] = 1;
  touched[v[i]] = 1;
}

__global__ __launch_bounds__(256) void k_e_touched_edges(const uint32_t* __restrict__ e_u, const uint32_t* __restrict__ e_v,
                                                         const uint8_t* __restrict__ e_alive, uint64_t ne,
                                                         const uint8_t* __restrict__ touched, uint64_t* __restrict__ flag)
{
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < ne) flag[e] = (e_alive[e] && touched[e_u[e]] && touched[e_v[e]]) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_e_set_u32(uint32_t* __restrict__ dst, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ val,
                                                   uint32_t constant, uint64_t n)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[idx[i]] = val ? val[i] : constant;
}

__global__ __launch_bounds__(256) void k_e_set_u8(uint8_t* __restrict__ dst, const uint32_t* __restrict__ idx, uint8_t value, uint64_t n)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[idx[i]] = value;
}

__global__ __launch_bounds__(256) void k_e_zero64_at(uint64_t* __restrict__ dst, const uint32_t* __restrict__ idx, uint64_t n)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[idx[i]] = 0;
}

__global__ __launch_bounds__(256) void k_e_not(uint64_t* __restrict__ f, uint64_t n)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) f[i] = f[i] ? 0 : 1;
}

__global__ __launch_bounds__(256) void k_e_append_edges(const uint64_t* __restrict__ keepf, const uint64_t* __restrict__ where, uint64_t lne,
                                                        const uint32_t* __restrict__ gu, const uint32_t* __restrict__ gv,
                                                        const uint32_t* __restrict__ lw, uint64_t ne0, uint32_t* __restrict__ e_u,
                                                        uint32_t* __restrict__ e_v, uint32_t* __restrict__ e_w, uint8_t* __restrict__ e_alive)
{
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= lne || (keepf && !keepf[e])) return;
  const uint64_t o = ne0 + (keepf ? where[e] : e);
  e_u[o] = gu[e];
  e_v[o] = gv[e];
  e_w[o] = lw[e];
  e_alive[o] = 1;
}

// ---- kernels: degrees, neighbours, deletions ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_e_degrees(const uint32_t* __restrict__ e_u, const uint32_t* __restrict__ e_v,
                                                   const uint8_t* __restrict__ e_alive, uint64_t ne, uint32_t* __restrict__ deg,
                                                   uint32_t* __restrict__ nbr, uint32_t* __restrict__ nbe)
{
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ne || !e_alive[e]) return;
  const uint32_t u = e_u[e], v = e_v[e];
  const uint32_t su = atomicAdd(&deg[u], 1u);
  if (nbr && su < 2) {
    nbr[2 * (uint64_t)u + su] = v;
    nbe[2 * (uint64_t)u + su] = (uint32_t)e;
  }
  const uint32_t sv = atomicAdd(&deg[v], 1u);
  if (nbr && sv < 2) {
    nbr[2 * (uint64_t)v + sv] = u;
    nbe[2 * (uint64_t)v + sv] = (uint32_t)e;
  }
}

__global__ __launch_bounds__(256) void k_e_kill(const uint8_t* __restrict__ dead, uint64_t nv, uint8_t* __restrict__ v_alive,
                                                const uint32_t* __restrict__ e_u, const uint32_t* __restrict__ e_v, uint64_t ne,
                                                uint8_t* __restrict__ e_alive)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nv && dead[i]) v_alive[i] = 0;
  if (i < ne && e_alive[i] && (dead[e_u[i]] || dead[e_v[i]])) e_alive[i] = 0;
}

// ---- kernels: bubbles, filter, erosion -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_e_bubble_cand(const uint32_t* __restrict__ e_u, const uint32_t* __restrict__ e_v,
                                                       const uint8_t* __restrict__ e_alive, uint64_t ne, const uint32_t* __restrict__ deg,
                                                       uint8_t* __restrict__ is_cv, uint64_t* __restrict__ flag)
{
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ne) return;
  const bool c = e_alive[e] && deg[e_u[e]] == 3 && deg[e_v[e]] == 3;
  flag[e] = c ? 1 : 0;
  if (c) {
    is_cv[e_u[e]] = 1;
    is_cv[e_v[e]] = 1;
  }
}

__global__ __launch_bounds__(256) void k_e_incident(const uint32_t* __restrict__ e_u, const uint32_t* __restrict__ e_v,
                                                    const uint8_t* __restrict__ e_alive, uint64_t ne, const uint8_t* __restrict__ is_cv,
                                                    uint64_t* __restrict__ flag)
{
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < ne) flag[e] = (e_alive[e] && (is_cv[e_u[e]] || is_cv[e_v[e]])) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_e_light(const uint32_t* __restrict__ e_w, uint8_t* __restrict__ e_alive, uint64_t ne, uint32_t min_w,
                                                 uint64_t* __restrict__ flag)
{
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ne) return;
  const bool light = e_alive[e] && e_w[e] < min_w;
  flag[e] = light ? 1 : 0;
  if (light) e_alive[e] = 0;
}

// erode_edges (S:312-340) for one flagged pair per lane; the walks read one snapshot of the graph and only mark edges,
// so they are independent of each other
__global__ __launch_bounds__(256) void k_e_erode(const uint32_t* __restrict__ fl_u, const uint32_t* __restrict__ fl_v, uint64_t n_flag,
                                                 const uint64_t* __restrict__ v_hash, const uint64_t* __restrict__ v_pos, uint64_t cap_v, uint32_t G,
                                                 const uint32_t* __restrict__ deg, const uint32_t* __restrict__ nbr,
                                                 const uint32_t* __restrict__ nbe, uint64_t k, uint8_t* __restrict__ e_dead,
                                                 uint32_t* __restrict__ later, unsigned long long* __restrict__ n_later, uint32_t all_later)
{
  // `later`: pairs whose walk this kernel cannot finish -- it meets a vertex with more than the two neighbours kept per vertex,
  // or visits more than MAXV vertices; the host walks those with the whole adjacency (nts_engine_erode).  Nothing of such a
  // pair is marked here.  all_later: every pair goes there (tests of that path).
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_flag) return;
  if (all_later) {
    later[atomicAdd(n_later, 1ULL)] = (uint32_t)i;
    return;
  }
  uint32_t s = fl_u[i], t = fl_v[i];
  if (dec_str_greater(v_hash[s], v_hash[t])) {
    const uint32_t x = s;
    s = t;
    t = x;
  }
  if (deg[s] != 1 || deg[t] != 1) return;
  auto too_close = [&](uint32_t a, uint32_t b) {
    for (uint32_t g = 0; g < G; ++g) {
      const uint64_t pa = v_pos[(uint64_t)g * cap_v + a], pb = v_pos[(uint64_t)g * cap_v + b];
      if ((pa > pb ? pa - pb : pb - pa) < k) return true;
    }
    return false;
  };
  constexpr int MAXV = 96;
  uint32_t visited[MAXV];
  int nvis = 0;
  visited[nvis++] = s;
  visited[nvis++] = t;
  // first the walk alone (can this kernel finish it?), then once more marking the edges
  for (int pass = 0; pass < 2; ++pass) {
    nvis = 2;
    bool erode_target = true;
    uint32_t cs = s, ct = t;
    while (too_close(cs, ct)) {
      const uint32_t v = erode_target ? ct : cs;
      const uint32_t d = deg[v];
      if (d > 2) { // more neighbours than are kept per vertex
        later[atomicAdd(n_later, 1ULL)] = (uint32_t)i;
        return;
      }
      uint32_t nxt = E_NONE;
      int n_nxt = 0;
      for (uint32_t q = 0; q < d; ++q) {
        if (pass) e_dead[nbe[2 * (uint64_t)v + q]] = 1;
        const uint32_t u = nbr[2 * (uint64_t)v + q];
        bool seen = false;
        for (int z = 0; z < nvis; ++z) seen |= visited[z] == u;
        if (!seen) {
          nxt = u;
          ++n_nxt;
        }
      }
      if (n_nxt == 0) break;
      if (n_nxt > 1 || nvis >= MAXV) { // (two ways on: the host reports it as the reference's assert does)
        later[atomicAdd(n_later, 1ULL)] = (uint32_t)i;
        return;
      }
      if (erode_target)
        ct = nxt;
      else
        cs = nxt;
      visited[nvis++] = nxt;
      erode_target = !erode_target;
    }
  }
}

__global__ __launch_bounds__(256) void k_e_mark_u8(const uint64_t* __restrict__ idx, uint64_t n, uint8_t* __restrict__ flags)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) flags[idx[i]] = 1;
}

__global__ __launch_bounds__(256) void k_e_apply_dead_edges(const uint8_t* __restrict__ e_dead, uint8_t* __restrict__ e_alive, uint64_t ne,
                                                            unsigned long long* __restrict__ count)
{
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool hit = e < ne && e_dead[e];
  if (hit) e_alive[e] = 0;
  const unsigned long long b = __ballot(hit);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, (unsigned long long)__popcll(b));
}

// ---- kernels: paths by list ranking ---------------------------------------------------------------------------------------
// An arc (v, d) = "at v, heading for v's d-th neighbour".  Following arcs through degree-2 vertices ends at a degree-1
// vertex (a path end) or at a branching vertex (which poisons the component, like ntJoin's find_paths only keeps
// components that are simple paths).  state = (next arc, hops so far, end vertex).
__global__ __launch_bounds__(256) void k_e_arc_init(const uint32_t* __restrict__ deg, const uint32_t* __restrict__ nbr, uint64_t nv,
                                                    uint4* __restrict__ st)
{
  const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= 2 * nv) return;
  const uint64_t v = x >> 1;
  const uint32_t d = (uint32_t)(x & 1);
  const uint32_t dg = deg[v];
  uint4 s = make_uint4(E_NONE, 0, E_BAD, 0);
  if ((dg == 1 || dg == 2) && d < dg) {
    const uint32_t u = nbr[2 * v + d];
    const uint32_t du = deg[u];
    s.y = 1;
    if (du == 1) {
      s.z = u;
    } else if (du == 2) {
      s.x = 2 * u + (nbr[2 * (uint64_t)u] == (uint32_t)v ? 1u : 0u);
      s.z = E_BAD;
    }
  }
  st[x] = s;
}

__global__ __launch_bounds__(256) void k_e_arc_jump(const uint4* __restrict__ in, uint4* __restrict__ out, uint64_t n_arcs)
{
  const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= n_arcs) return;
  uint4 s = in[x];
  if (s.x != E_NONE) {
    const uint4 t = in[s.x];
    s.y += t.y;
    s.z = t.z;
    s.x = t.x;
  }
  out[x] = s;
}

// per vertex: is it on a simple path, which end does the path start at (the end with the smaller position in the
// reference assembly -- ntJoin's determine_source_vertex; ties keep the smaller vertex id first, as nts_walk_paths does),
// and its index from there
__global__ __launch_bounds__(256) void k_e_classify(const uint32_t* __restrict__ deg, const uint4* __restrict__ st, uint64_t nv,
                                                    const uint64_t* __restrict__ key, uint32_t* __restrict__ pstart, uint32_t* __restrict__ pidx,
                                                    uint32_t* __restrict__ plen, uint64_t* __restrict__ is_start)
{
  const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv) return;
  const uint32_t dg = deg[v];
  uint32_t ps = E_NONE, idx = 0, len = 0;
  if (dg == 1) {
    const uint4 s0 = st[2 * v];
    if (s0.x == E_NONE && s0.z != E_BAD) {
      const uint32_t A = (uint32_t)v, B = s0.z;
      const uint32_t lo = A < B ? A : B, hi = A < B ? B : A;
      ps = key[hi] < key[lo] ? hi : lo;
      len = s0.y + 1;
      idx = ps == A ? 0 : len - 1;
    }
  } else if (dg == 2) {
    const uint4 s0 = st[2 * v], s1 = st[2 * v + 1];
    if (s0.x == E_NONE && s1.x == E_NONE && s0.z != E_BAD && s1.z != E_BAD && s0.z != s1.z) {
      const uint32_t A = s0.z, B = s1.z;
      const uint32_t lo = A < B ? A : B, hi = A < B ? B : A;
      ps = key[hi] < key[lo] ? hi : lo;
      len = s0.y + s1.y + 1;
      idx = ps == A ? s0.y : s1.y;
    }
  }
  pstart[v] = ps;
  pidx[v] = idx;
  plen[v] = len;
  is_start[v] = (ps == (uint32_t)v) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_e_path_len(const uint64_t* __restrict__ is_start, const uint64_t* __restrict__ pnum,
                                                    const uint32_t* __restrict__ plen, uint64_t nv, uint64_t* __restrict__ lens)
{
  const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v < nv && is_start[v]) lens[pnum[v]] = plen[v];
}

__global__ __launch_bounds__(256) void k_e_place(const uint32_t* __restrict__ pstart, const uint32_t* __restrict__ pidx,
                                                 const uint64_t* __restrict__ pnum, const uint64_t* __restrict__ poff, uint64_t nv,
                                                 uint32_t* __restrict__ verts, uint32_t* __restrict__ vpath)
{
  const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv || pstart[v] == E_NONE) return;
  const uint64_t p = pnum[pstart[v]];
  const uint64_t j = poff[p] + pidx[v];
  verts[j] = (uint32_t)v;
  vpath[j] = (uint32_t)p;
}

// ---- kernels: blocks of paths (rows C6-C9) ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_e_run_init(const uint64_t* __restrict__ poff, uint64_t n_paths, uint32_t* __restrict__ pst)
{
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n_paths) pst[p] = (uint32_t)poff[p];
}

// a path whose contig changes in any assembly keeps only its last run (S:71-77)
__global__ __launch_bounds__(256) void k_e_run_start(const uint32_t* __restrict__ verts, const uint32_t* __restrict__ vpath, uint64_t N,
                                                     const uint64_t* __restrict__ poff, const uint32_t* __restrict__ v_rec, uint64_t cap_v,
                                                     uint32_t G, uint32_t* __restrict__ pst)
{
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= N) return;
  const uint32_t p = vpath[j];
  if (j == poff[p]) return;
  const uint32_t x = verts[j - 1], y = verts[j];
  bool change = false;
  for (uint32_t a = 0; a < G; ++a) change |= v_rec[(uint64_t)a * cap_v + x] != v_rec[(uint64_t)a * cap_v + y];
  if (change) atomicMax(&pst[p], (uint32_t)j);
}

// rising steps per assembly over the kept run (synteny_block.py:48-65) and indel flags (S:364-409).  The lanes of a wave hold
// consecutive path positions, nearly always of one path: the rising steps are counted with a ballot per (path, assembly) and
// added by one lane (one atomic per lane piled 6 M additions on 72 counters at human scale: 81 ms; now well under one).
__global__ __launch_bounds__(256) void k_e_steps(const uint32_t* __restrict__ verts, const uint32_t* __restrict__ vpath, uint64_t N,
                                                 const uint64_t* __restrict__ poff, const uint32_t* __restrict__ pst,
                                                 const uint64_t* __restrict__ v_pos, uint64_t cap_v, uint32_t G, uint64_t n_paths, int64_t bp,
                                                 uint32_t* __restrict__ n_up, uint8_t* __restrict__ over)
{
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool inside = j < N;
  const uint32_t p = inside ? vpath[j] : 0u;
  const bool step = inside && j >= pst[p] && j + 1 < poff[p + 1];
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t x = 0, y = 0;
  if (step) {
    x = verts[j];
    y = verts[j + 1];
  }
  int64_t g_min = INT64_MAX, g_max = INT64_MIN;
  for (uint32_t a = 0; a < G; ++a) {
    bool up = false;
    if (step) {
      const int64_t px = (int64_t)v_pos[(uint64_t)a * cap_v + x], py = (int64_t)v_pos[(uint64_t)a * cap_v + y];
      up = py > px;
      const int64_t g = px > py ? px - py : py - px;
      g_min = g < g_min ? g : g_min;
      g_max = g > g_max ? g : g_max;
    }
    unsigned long long todo = __ballot(step);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const uint32_t pl = (uint32_t)__shfl((int)p, leader, 64);
      const unsigned long long same = __ballot(step && p == pl);
      const unsigned long long ups = __ballot(step && p == pl && up);
      if ((int)lane == leader && ups) atomicAdd(&n_up[(uint64_t)a * n_paths + pl], (uint32_t)__popcll(ups));
      todo &= ~same;
    }
  }
  if (inside) over[j] = (step && g_max - g_min > bp) ? 1 : 0;
}

// determine_orientations + all_oriented (synteny_block.py:48-70): 0 '+', 1 '-', 2 '?'
__global__ __launch_bounds__(256) void k_e_orient(const uint64_t* __restrict__ poff, const uint32_t* __restrict__ pst,
                                                  const uint32_t* __restrict__ n_up, uint64_t n_paths, uint32_t G, double m,
                                                  uint8_t* __restrict__ pcode, uint8_t* __restrict__ pgood, unsigned long long* __restrict__ n_bad)
{
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_paths) return;
  const uint64_t n_d = poff[p + 1] - pst[p] - 1;
  bool good = true;
  for (uint32_t a = 0; a < G; ++a) {
    const uint64_t up = n_up[(uint64_t)a * n_paths + p];
    const double pos_perc = (double)up / (double)n_d * 100.0;
    const double neg_perc = 100.0 - pos_perc;
    uint8_t c = 2;
    if (neg_perc >= m) c = 1;
    if (pos_perc >= m) c = 0;
    if (up == 0) c = 1;
    if (up == n_d) c = 0; // includes single-vertex runs
    pcode[(uint64_t)a * n_paths + p] = c;
    good &= c != 2;
  }
  pgood[p] = good ? 1 : 0;
  if (!good) atomicAdd(n_bad, 1ull);
}

// blocks without an orientation are dropped with their vertices (S:84-86, S:96-104); block boundaries at indel cuts
__global__ __launch_bounds__(256) void k_e_block_starts(const uint32_t* __restrict__ verts, const uint32_t* __restrict__ vpath, uint64_t N,
                                                        const uint64_t* __restrict__ poff, const uint32_t* __restrict__ pst,
                                                        const uint8_t* __restrict__ pgood, uint8_t* __restrict__ over,
                                                        uint8_t* __restrict__ dead, uint64_t* __restrict__ bstart)
{
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= N) return;
  const uint32_t p = vpath[j];
  const bool in_run = j >= pst[p];
  uint64_t b = 0;
  if (!pgood[p]) {
    over[j] = 0;
    if (in_run) dead[verts[j]] = 1;
  } else if (in_run) {
    b = (j == pst[p] || over[j - 1]) ? 1 : 0;
  }
  bstart[j] = b;
}

// (runs after k_e_block_starts, which clears the flags of paths without an orientation)
__global__ __launch_bounds__(256) void k_e_cuts(const uint32_t* __restrict__ verts, uint64_t N, const uint8_t* __restrict__ over,
                                                const uint32_t* __restrict__ nbr, const uint32_t* __restrict__ nbe, uint8_t* __restrict__ e_alive,
                                                unsigned long long* __restrict__ n_cuts)
{
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool cut = j < N && over[j];
  if (cut) {
    const uint32_t x = verts[j], y = verts[j + 1];
    const uint32_t e = nbr[2 * (uint64_t)x] == y ? nbe[2 * (uint64_t)x] : nbe[2 * (uint64_t)x + 1];
    e_alive[e] = 0;
  }
  const unsigned long long b = __ballot(cut);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(n_cuts, (unsigned long long)__popcll(b));
}

__global__ __launch_bounds__(256) void k_e_block_bounds(const uint32_t* __restrict__ vpath, uint64_t N, const uint64_t* __restrict__ poff,
                                                        const uint32_t* __restrict__ pst, const uint8_t* __restrict__ pgood,
                                                        const uint8_t* __restrict__ over, const uint64_t* __restrict__ bstart,
                                                        const uint64_t* __restrict__ bscan, uint32_t* __restrict__ bfirst,
                                                        uint32_t* __restrict__ blast, uint32_t* __restrict__ bpath)
{
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= N) return;
  const uint32_t p = vpath[j];
  if (!pgood[p] || j < pst[p]) return;
  const uint64_t b = bscan[j] + bstart[j] - 1;
  if (bstart[j]) {
    bfirst[b] = (uint32_t)j;
    bpath[b] = p;
  }
  if (j + 1 == poff[p + 1] || over[j]) blast[b] = (uint32_t)j;
}

// filter_synteny_blocks(paths, min_mx) (S:411-426)
__global__ __launch_bounds__(256) void k_e_block_keep(const uint32_t* __restrict__ bfirst, const uint32_t* __restrict__ blast, uint64_t n_blocks,
                                                      uint32_t min_mx, uint64_t* __restrict__ bkeep, unsigned long long* __restrict__ n_small)
{
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_blocks) return;
  const bool keep = blast[b] - bfirst[b] + 1 >= min_mx;
  bkeep[b] = keep ? 1 : 0;
  if (!keep) atomicAdd(n_small, 1ull);
}

__global__ __launch_bounds__(256) void k_e_block_marks(const uint32_t* __restrict__ verts, const uint32_t* __restrict__ vpath, uint64_t N,
                                                       const uint32_t* __restrict__ pst, const uint8_t* __restrict__ pgood,
                                                       const uint64_t* __restrict__ bstart, const uint64_t* __restrict__ bscan,
                                                       const uint64_t* __restrict__ bkeep, const uint32_t* __restrict__ bfirst,
                                                       const uint32_t* __restrict__ blast, uint8_t* __restrict__ dead,
                                                       uint8_t* __restrict__ internal, uint8_t* __restrict__ terminal)
{
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= N) return;
  const uint32_t p = vpath[j];
  if (!pgood[p] || j < pst[p]) return;
  const uint64_t b = bscan[j] + bstart[j] - 1;
  const uint32_t v = verts[j];
  if (!bkeep[b])
    dead[v] = 1;
  else if (j == bfirst[b] || j == blast[b])
    terminal[v] = 1;
  else
    internal[v] = 1;
}

__global__ __launch_bounds__(256) void k_e_block_table(const uint64_t* __restrict__ bkeep, const uint64_t* __restrict__ bwhere, uint64_t n_blocks,
                                                       uint64_t n_kept, const uint32_t* __restrict__ bfirst, const uint32_t* __restrict__ blast,
                                                       const uint32_t* __restrict__ bpath, const uint32_t* __restrict__ verts,
                                                       const uint32_t* __restrict__ pst, const uint8_t* __restrict__ pcode, uint64_t n_paths,
                                                       const uint32_t* __restrict__ v_rec, const uint64_t* __restrict__ v_pos, uint64_t cap_v,
                                                       uint32_t G, uint32_t* __restrict__ o_first, uint32_t* __restrict__ o_last,
                                                       uint32_t* __restrict__ o_n, uint32_t* __restrict__ o_rec, uint64_t* __restrict__ o_fp,
                                                       uint64_t* __restrict__ o_lp, uint8_t* __restrict__ o_ori)
{
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_blocks || !bkeep[b]) return;
  const uint64_t o = bwhere[b];
  const uint32_t p = bpath[b];
  const uint32_t fv = verts[bfirst[b]], lv = verts[blast[b]], head = verts[pst[p]];
  o_first[o] = fv;
  o_last[o] = lv;
  o_n[o] = blast[b] - bfirst[b] + 1;
  for (uint32_t a = 0; a < G; ++a) {
    o_rec[(uint64_t)a * n_kept + o] = v_rec[(uint64_t)a * cap_v + head]; // contig / orientation inherited from the path (S:383)
    o_fp[(uint64_t)a * n_kept + o] = v_pos[(uint64_t)a * cap_v + fv];
    o_lp[(uint64_t)a * n_kept + o] = v_pos[(uint64_t)a * cap_v + lv];
    o_ori[(uint64_t)a * n_kept + o] = pcode[(uint64_t)a * n_paths + p];
  }
}

// slice bounds of a (record, position)-ordered list: cut[i] = first element whose record is >= base[i]
__global__ __launch_bounds__(256) void k_e_rec_bounds(const uint32_t* __restrict__ rec, uint64_t n, const uint32_t* __restrict__ base,
                                                      uint32_t n_bounds, uint64_t* __restrict__ cut)
{
  for (uint32_t i = threadIdx.x; i < n_bounds; i += blockDim.x) {
    const uint32_t x = base[i];
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (rec[mid] < x)
        lo = mid + 1;
      else
        hi = mid;
    }
    cut[i] = lo;
  }
}

__global__ __launch_bounds__(256) void k_e_rebase(const uint32_t* __restrict__ rec, uint64_t n, uint32_t base, uint32_t* __restrict__ out)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = rec[i] - base;
}

// ---- host-side pieces ------------------------------------------------------------------------------------------------------
int e_scan(nts_ctx* ctx, const uint64_t* in, uint64_t* out, uint64_t n, bool inclusive = false)
{
  size_t tmp = 0;
  if (inclusive)
    HIP_TRY(ctx, rocprim::inclusive_scan(nullptr, tmp, in, out, n, rocprim::plus<uint64_t>(), ctx->stream));
  else
    HIP_TRY(ctx, rocprim::exclusive_scan(nullptr, tmp, in, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), ctx->stream));
  void* d_tmp = ws_get(ctx, "e_scan_tmp", std::max<size_t>(tmp, 16));
  if (!d_tmp) return NTS_ENOMEM;
  if (inclusive)
    HIP_TRY(ctx, rocprim::inclusive_scan(d_tmp, tmp, in, out, n, rocprim::plus<uint64_t>(), ctx->stream));
  else
    HIP_TRY(ctx, rocprim::exclusive_scan(d_tmp, tmp, in, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), ctx->stream));
  return NTS_OK;
}

int e_degrees(nts_ctx* ctx, nts_engine* E, uint32_t** deg, uint32_t** nbr, uint32_t** nbe)
{
  const uint64_t nv = std::max<uint64_t>(E->nv, 1);
  NTS_WS(d_deg, uint32_t*, "e_deg", nv * 4);
  HIP_TRY(ctx, hipMemsetAsync(d_deg, 0, nv * 4, ctx->stream));
  uint32_t *d_nbr = nullptr, *d_nbe = nullptr;
  if (nbr) {
    d_nbr = (uint32_t*)ws_get(ctx, "e_nbr", nv * 8);
    d_nbe = (uint32_t*)ws_get(ctx, "e_nbe", nv * 8);
    if (!d_nbr || !d_nbe) return NTS_ENOMEM;
    HIP_TRY(ctx, hipMemsetAsync(d_nbr, 0xFF, nv * 8, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_nbe, 0xFF, nv * 8, ctx->stream));
  }
  if (E->ne) NTS_LAUNCH(k_e_degrees, E_GRID(E->ne), E->e_u, E->e_v, E->e_alive, E->ne, d_deg, d_nbr, d_nbe);
  HIP_TRY(ctx, hipGetLastError());
  *deg = d_deg;
  if (nbr) {
    *nbr = d_nbr;
    *nbe = d_nbe;
  }
  return NTS_OK;
}

// the position filters of a refinement round as the graph build's list hook
struct RefineHook : ListHook
{
  const uint64_t *cs, *cm, *iv_off;
  int operator()(nts_ctx* ctx, uint64_t n, const uint8_t* d_valid, const uint32_t* d_asm, const uint32_t* d_rec, const uint64_t* d_pos,
                 uint32_t* d_list) override
  {
    NTS_WS(d_a, uint64_t*, "e_hook_a", n * 8);
    NTS_WS(d_b, uint64_t*, "e_hook_b", n * 8);
    NTS_LAUNCH(k_e_lastvalid_in, E_GRID(n), d_valid, n, d_a);
    size_t tmp = 0;
    HIP_TRY(ctx, rocprim::inclusive_scan(nullptr, tmp, d_a, d_b, n, rocprim::maximum<uint64_t>(), ctx->stream));
    void* d_tmp = ws_get(ctx, "e_scan_tmp", std::max<size_t>(tmp, 16));
    if (!d_tmp) return NTS_ENOMEM;
    HIP_TRY(ctx, rocprim::inclusive_scan(d_tmp, tmp, d_a, d_b, n, rocprim::maximum<uint64_t>(), ctx->stream));
    NTS_LAUNCH(k_e_newlist, E_GRID(n), d_valid, d_b, d_asm, d_rec, d_pos, n, cs, cm, iv_off, d_a);
    if (int rc = e_scan(ctx, d_a, d_b, n, true)) return rc;
    NTS_LAUNCH(k_e_listid, E_GRID(n), d_b, n, d_list);
    HIP_TRY(ctx, hipGetLastError());
    return NTS_OK;
  }
};

// ntJoin's read_minimizers with a repeat filter (stage 3's `--filter Filter`, bin/ntsynt_synteny.py:183-184,601-604): a minimizer whose
// k-mer the filter holds is not read.  One lane per minimizer: canonical ntHash of its k bases (one byte per base in the genome's code
// array, base by base -- a few million k-mers per list), h0 mod bits, one probe; keep[i] = 1 when the filter does not hold it.
__global__ __launch_bounds__(256) void k_mx_screen_flags(const uint8_t* __restrict__ code, const uint64_t* __restrict__ rec_off, const uint32_t* __restrict__ rec,
                                                        const uint64_t* __restrict__ pos, uint64_t n, HashParams hp, const uint32_t* __restrict__ bf, FastMod fm,
                                                        uint32_t* __restrict__ keep)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t* s = code + rec_off[rec[i]] + pos[i];
  const uint32_t k = hp.k;
  uint64_t f = 0, r = 0;
  bool valid = true;
  for (uint32_t q = 0; q < k; ++q) {
    const uint32_t a = s[q], b = s[k - 1u - q];
    valid &= a < 4u;
    f = srol1(f) ^ hp.seed[a & 3u];
    r = srol1(r) ^ hp.seed[3u - (b & 3u)];
  }
  // (a minimizer's k-mer holds no other byte than A, C, G, T; one that did would be kept: the filter cannot hold it)
  keep[i] = (valid && bf_test(bf, fm(f + r))) ? 0u : 1u;
}

__global__ __launch_bounds__(256) void k_mx_screen_move(const uint64_t* __restrict__ h1, const uint32_t* __restrict__ rec, const uint64_t* __restrict__ pos,
                                                       const uint32_t* __restrict__ keep, const uint64_t* __restrict__ at, uint64_t n,
                                                       uint64_t* __restrict__ o_h1, uint32_t* __restrict__ o_rec, uint64_t* __restrict__ o_pos)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !keep[i]) return;
  const uint64_t o = at[i];
  o_h1[o] = h1[i];
  o_rec[o] = rec[i];
  o_pos[o] = pos[i];
}

} // namespace

extern "C" {

int nts_engine_create(nts_ctx* ctx, uint32_t n_asm, uint32_t ref_asm, nts_engine** out)
{
  if (!ctx || !out || n_asm == 0 || ref_asm >= n_asm) return fail(ctx, NTS_EINVAL, "nts_engine_create: bad arguments");
  nts_engine* E = new nts_engine();
  E->G = n_asm;
  E->ref = ref_asm;
  *out = E;
  return NTS_OK;
}

void nts_engine_free(nts_ctx* ctx, nts_engine* E)
{
  if (!E) return;
  if (ctx) hipSetDevice(ctx->device);
  dev_free(E->v_hash);
  dev_free(E->v_alive);
  dev_free(E->v_rec);
  dev_free(E->v_pos);
  dev_free(E->internal);
  dev_free(E->terminal);
  dev_free(E->e_u);
  dev_free(E->e_v);
  dev_free(E->e_w);
  dev_free(E->e_alive);
  dev_free(E->fl_u);
  dev_free(E->fl_v);
  delete E;
}

int nts_engine_size(const nts_engine* E, uint64_t* nv, uint64_t* ne)
{
  if (!E) return NTS_EINVAL;
  if (nv) *nv = E->nv;
  if (ne) *ne = E->ne;
  return NTS_OK;
}

// Field read-back for tests and debugging: "v_hash" u64[nv], "v_alive" u8[nv], "v_rec" u32[G*nv], "v_pos" u64[G*nv], "internal" /
// "terminal" u8[nv], "e_u" / "e_v" / "e_w" u32[ne], "e_alive" u8[ne]; after nts_engine_blocks also "path_verts" u32[n] and
// "path_off" u64[n_paths+1] (sizes through nts_engine_paths).
int nts_engine_read(nts_ctx* ctx, const nts_engine* E, const char* field, void* dst, uint64_t bytes)
{
  if (!ctx || !E || !field || (!dst && bytes)) return fail(ctx, NTS_EINVAL, "nts_engine_read: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const std::string f(field);
  auto plain = [&](const void* src, uint64_t n) -> int {
    if (bytes != n) return fail(ctx, NTS_EINVAL, "nts_engine_read: size mismatch for " + f);
    if (n) HIP_TRY(ctx, hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NTS_OK;
  };
  if (f == "v_hash") return plain(E->v_hash, E->nv * 8);
  if (f == "v_alive") return plain(E->v_alive, E->nv);
  if (f == "internal") return plain(E->internal, E->nv);
  if (f == "terminal") return plain(E->terminal, E->nv);
  if (f == "e_u") return plain(E->e_u, E->ne * 4);
  if (f == "e_v") return plain(E->e_v, E->ne * 4);
  if (f == "e_w") return plain(E->e_w, E->ne * 4);
  if (f == "e_alive") return plain(E->e_alive, E->ne);
  if (f == "v_rec" || f == "v_pos") {
    const uint64_t w = f == "v_rec" ? 4 : 8;
    if (bytes != (uint64_t)E->G * E->nv * w) return fail(ctx, NTS_EINVAL, "nts_engine_read: size mismatch for " + f);
    for (uint32_t a = 0; a < E->G && E->nv; ++a) {
      const uint8_t* src = (f == "v_rec" ? (const uint8_t*)E->v_rec : (const uint8_t*)E->v_pos) + (uint64_t)a * E->cap_v * w;
      HIP_TRY(ctx, hipMemcpyAsync((uint8_t*)dst + (uint64_t)a * E->nv * w, src, E->nv * w, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NTS_OK;
  }
  if (f == "path_verts") return plain(ctx->ws["e_verts"].first, E->n_path_verts * 4);
  if (f == "path_off") return plain(ctx->ws["e_poff"].first, (E->n_paths + 1) * 8);
  return fail(ctx, NTS_EINVAL, "nts_engine_read: unknown field " + f);
}

int nts_engine_paths(const nts_engine* E, uint64_t* n_paths, uint64_t* n_verts)
{
  if (!E) return NTS_EINVAL;
  if (n_paths) *n_paths = E->n_paths;
  if (n_verts) *n_verts = E->n_path_verts;
  return NTS_OK;
}

// One build into the engine.  lists[a]: the round's minimizer list of assembly a (reference order: descending file name),
// resident in HBM.  spans == NULL: the initial round (S:607-612).  Otherwise a refinement round (S:476-491): spans[a] holds
// the block interiors of assembly a as composite keys record * 2^40 + position, sorted by start (`start`), with the running
// maximum of the composite ends (`end_max`) -- what ntsynt_amd/synteny.py builds for its own `overlaps`; new minimizers that
// are internal to a block (by hash, using the marks of the last nts_engine_blocks call) or positioned in a block interior
// are dropped, lists are cut where they cross an interior, terminals keep their vertices.
int nts_engine_add(nts_ctx* ctx, nts_engine* E, const nts_mx* const* lists, const nts_spans* spans, uint64_t* nv_out, uint64_t* ne_out)
{
  if (!ctx || !E || !lists) return fail(ctx, NTS_EINVAL, "nts_engine_add: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ctx->graph_live0 = nts_mem::live.load();
  const uint32_t G = E->G;
  uint64_t n = 0;
  for (uint32_t a = 0; a < G; ++a) {
    if (!lists[a]) return fail(ctx, NTS_EINVAL, "nts_engine_add: NULL list");
    n += lists[a]->n;
  }
  if (n >= 0xFFFFFFF0ULL) return fail(ctx, NTS_ERANGE, "nts_engine_add: more than 2^32 minimizers");
  if (nv_out) *nv_out = E->nv;
  if (ne_out) *ne_out = E->ne;
  if (n == 0) return NTS_OK;
  GraphIn in;
  if (graph_inputs(ctx, n, &in) != NTS_OK) return NTS_ENOMEM;
  uint64_t o = 0;
  for (uint32_t a = 0; a < G; ++a) {
    const uint64_t m = lists[a]->n;
    if (m) {
      HIP_TRY(ctx, hipMemcpyAsync(in.h + o, lists[a]->d_h1, m * 8, hipMemcpyDeviceToDevice, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(in.rec + o, lists[a]->d_rec, m * 4, hipMemcpyDeviceToDevice, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(in.pos + o, lists[a]->d_pos, m * 8, hipMemcpyDeviceToDevice, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(in.list + o, lists[a]->d_rec, m * 4, hipMemcpyDeviceToDevice, ctx->stream));
      HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)(in.asm_id + o), (int)a, m, ctx->stream));
    }
    o += m;
  }
  HIP_TRY(ctx, hipMemsetAsync(in.keep, 1, n, ctx->stream));
  const uint64_t nv0 = E->nv, ne0 = E->ne;
  uint64_t* d_hs = nullptr;
  uint32_t* d_hid = nullptr;
  uint64_t nl = 0;
  RefineHook hook;
  const bool refine = spans != nullptr;
  if (nv0) {
    // live index: (hash, vertex) of the live vertices, by hash -- a deleted vertex may share its hash with a re-created one
    NTS_WS(d_f, uint64_t*, "e_flag", nv0 * 8);
    NTS_WS(d_s, uint64_t*, "e_scan", nv0 * 8);
    NTS_WS(d_k, uint64_t*, "e_hs0", nv0 * 8);
    NTS_WS(d_i, uint32_t*, "e_hid0", nv0 * 4);
    d_hs = (uint64_t*)ws_get(ctx, "e_hs", nv0 * 8);
    d_hid = (uint32_t*)ws_get(ctx, "e_hid", nv0 * 4);
    if (!d_hs || !d_hid) return NTS_ENOMEM;
    NTS_LAUNCH(k_e_live_flag, E_GRID(nv0), E->v_alive, nv0, d_f);
    if (int rc = e_scan(ctx, d_f, d_s, nv0)) return rc;
    if (int rc = flag_count(ctx, d_f, d_s, nv0, &nl)) return rc;
    NTS_LAUNCH(k_e_live_pairs, E_GRID(nv0), E->v_alive, d_s, E->v_hash, nv0, d_k, d_i);
    if (nl) {
      size_t tmp = 0;
      HIP_TRY(ctx, rocprim::radix_sort_pairs(nullptr, tmp, d_k, d_hs, d_i, d_hid, nl, 0, 64, ctx->stream));
      void* d_tmp = ws_get(ctx, "e_sort_tmp", std::max<size_t>(tmp, 16));
      if (!d_tmp) return NTS_ENOMEM;
      HIP_TRY(ctx, rocprim::radix_sort_pairs(d_tmp, tmp, d_k, d_hs, d_i, d_hid, nl, 0, 64, ctx->stream));
    }
  }
  if (refine) {
    // the block interiors of every assembly, one after the other
    std::vector<uint64_t> off(G + 1, 0);
    for (uint32_t a = 0; a < G; ++a) off[a + 1] = off[a] + spans[a].n;
    const uint64_t tot = off[G];
    NTS_WS(d_cs, uint64_t*, "e_iv_s", tot * 8);
    NTS_WS(d_cm, uint64_t*, "e_iv_m", tot * 8);
    NTS_WS(d_off, uint64_t*, "e_iv_off", (G + 1) * 8);
    for (uint32_t a = 0; a < G; ++a) {
      if (!spans[a].n) continue;
      if (!spans[a].start || !spans[a].end_max) return fail(ctx, NTS_EINVAL, "nts_engine_add: NULL span arrays");
      HIP_TRY(ctx, hipMemcpyAsync(d_cs + off[a], spans[a].start, spans[a].n * 8, hipMemcpyHostToDevice, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(d_cm + off[a], spans[a].end_max, spans[a].n * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(ctx, hipMemcpyAsync(d_off, off.data(), (G + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // `off` is a host temporary
    hook.cs = d_cs;
    hook.cm = d_cm;
    hook.iv_off = d_off;
    NTS_LAUNCH(k_e_keep, E_GRID(n), in.h, in.asm_id, in.rec, in.pos, n, d_hs, d_hid, nl, E->internal, d_cs, d_cm, d_off, in.keep);
  }
  GraphDev GD;
  if (int rc = graph_build_core(ctx, G, n, &GD, refine ? &hook : nullptr)) return rc;
  const uint64_t lnv = GD.nv, lne = GD.ne;
  if (lnv == 0) return NTS_OK;
  // ---- vertices
  NTS_WS(d_l2g, uint32_t*, "e_l2g", lnv * 4);
  NTS_WS(d_new, uint64_t*, "e_new", lnv * 8);
  NTS_WS(d_rank, uint64_t*, "e_rank", lnv * 8);
  uint64_t n_new = lnv;
  if (nv0) {
    NTS_LAUNCH(k_e_lookup, E_GRID(lnv), GD.v_hash, lnv, d_hs, d_hid, nl, d_l2g, d_new);
    if (int rc = e_scan(ctx, d_new, d_rank, lnv)) return rc;
    if (int rc = flag_count(ctx, d_new, d_rank, lnv, &n_new)) return rc;
  } else {
    HIP_TRY(ctx, hipMemsetAsync(d_l2g, 0xFF, lnv * 4, ctx->stream));
    // rank = the local id: fill through a scan of ones
    HIP_TRY(ctx, hipMemsetAsync(d_new, 0, lnv * 8, ctx->stream));
    NTS_LAUNCH(k_e_not, E_GRID(lnv), d_new, lnv);
    if (int rc = e_scan(ctx, d_new, d_rank, lnv)) return rc;
  }
  if (nv0 + n_new >= 0xFFFFFFF0ULL) return fail(ctx, NTS_ERANGE, "nts_engine_add: more than 2^32 vertices");
  if (int rc = e_reserve_vertices(ctx, E, nv0 + n_new)) return rc;
  NTS_LAUNCH(k_e_put_vertices, E_GRID(lnv), GD.v_hash, GD.occ_rec, GD.occ_pos, lnv, G, d_l2g, d_rank, nv0, E->cap_v, E->v_hash,
                     E->v_alive, E->internal, E->terminal, E->v_rec, E->v_pos);
  E->nv = nv0 + n_new;
  // ---- edges (already in ntJoin's dict order)
  if (lne) {
    NTS_WS(d_gu, uint32_t*, "e_gu", lne * 4);
    NTS_WS(d_gv, uint32_t*, "e_gv", lne * 4);
    NTS_WS(d_oo, uint64_t*, "e_oo", lne * 8);
    NTS_WS(d_oos, uint64_t*, "e_oos", lne * 8);
    NTS_LAUNCH(k_e_map_edges, E_GRID(lne), GD.e_u, GD.e_v, lne, d_l2g, nv0, d_gu, d_gv, d_oo);
    uint64_t n_oo = 0;
    if (nv0 && ne0) {
      if (int rc = e_scan(ctx, d_oo, d_oos, lne)) return rc;
      if (int rc = flag_count(ctx, d_oo, d_oos, lne, &n_oo)) return rc;
    }
    uint64_t n_dup = 0;
    if (n_oo) {
      // an edge that already exists (alive) keeps its slot and takes the new weight; only an edge between two vertices that
      // existed before this build can be one.  The candidates and the live edges among their end points are few: joined on
      // the host.
      NTS_WS(q_idx, uint32_t*, "e_q_idx", n_oo * 4);
      NTS_WS(q_u, uint32_t*, "e_q_u", n_oo * 4);
      NTS_WS(q_v, uint32_t*, "e_q_v", n_oo * 4);
      NTS_WS(q_w, uint32_t*, "e_q_w", n_oo * 4);
      NTS_LAUNCH(k_e_take_flagged, E_GRID(lne), d_oo, d_oos, lne, d_gu, d_gv, GD.e_w, q_idx, q_u, q_v, q_w);
      NTS_WS(d_touched, uint8_t*, "e_touched", nv0);
      HIP_TRY(ctx, hipMemsetAsync(d_touched, 0, nv0, ctx->stream));
      NTS_LAUNCH(k_e_touch, E_GRID(n_oo), q_u, q_v, n_oo, d_touched);
      NTS_WS(d_tf, uint64_t*, "e_flag", std::max(ne0, nv0) * 8);
      NTS_WS(d_ts, uint64_t*, "e_scan", std::max(ne0, nv0) * 8);
      NTS_LAUNCH(k_e_touched_edges, E_GRID(ne0), E->e_u, E->e_v, E->e_alive, ne0, d_touched, d_tf);
      if (int rc = e_scan(ctx, d_tf, d_ts, ne0)) return rc;
      uint64_t n_te = 0;
      if (int rc = flag_count(ctx, d_tf, d_ts, ne0, &n_te)) return rc;
      if (n_te) {
        NTS_WS(t_idx, uint32_t*, "e_t_idx", n_te * 4);
        NTS_WS(t_u, uint32_t*, "e_t_u", n_te * 4);
        NTS_WS(t_v, uint32_t*, "e_t_v", n_te * 4);
        NTS_LAUNCH(k_e_take_flagged, E_GRID(ne0), d_tf, d_ts, ne0, E->e_u, E->e_v, (const uint32_t*)nullptr, t_idx, t_u, t_v,
                           (uint32_t*)nullptr);
        // the join on the device: the live edges' pairs sorted (stable: of two live edges of one pair -- which cannot be -- the older comes
        // first, as the host-side dictionary this replaces kept it), every new edge looked up.  (Dense sketches make both sides large: w = 64 on
        // 3 x 1 Gbp, second refinement round: 10.5 M new edges between old vertices against 13.6 M live edges -- 20 s through a std::map.)
        if (NTS_KNOB("NTS_DEBUG_ENGINE")) fprintf(stderr, "[engine add] new edges between old vertices %llu, live edges at their ends %llu (of %llu edges, %llu new)\n",
                                                  (unsigned long long)n_oo, (unsigned long long)n_te, (unsigned long long)ne0, (unsigned long long)lne);
        NTS_WS(d_tk, uint64_t*, "e_join_key", n_te * 8);
        NTS_WS(d_tk2, uint64_t*, "e_join_key2", n_te * 8);
        NTS_WS(t_idx2, uint32_t*, "e_join_idx2", n_te * 4);
        NTS_LAUNCH(k_e_pair_keys, E_GRID(n_te), t_u, t_v, n_te, d_tk);
        {
          size_t tmp = 0;
          HIP_TRY(ctx, rocprim::radix_sort_pairs(nullptr, tmp, d_tk, d_tk2, t_idx, t_idx2, n_te, 0, 64, ctx->stream));
          void* d_tmp = ws_get(ctx, "e_join_tmp", std::max<size_t>(tmp, 16));
          if (!d_tmp) return NTS_ENOMEM;
          HIP_TRY(ctx, rocprim::radix_sort_pairs(d_tmp, tmp, d_tk, d_tk2, t_idx, t_idx2, n_te, 0, 64, ctx->stream));
        }
        NTS_WS(d_hit, uint64_t*, "e_join_hit", n_oo * 8);
        NTS_WS(d_hits, uint64_t*, "e_join_hits", n_oo * 8);
        NTS_WS(d_hedge, uint32_t*, "e_join_edge", n_oo * 4);
        NTS_LAUNCH(k_e_join_pairs, E_GRID(n_oo), q_u, q_v, n_oo, d_tk2, t_idx2, n_te, d_hit, d_hedge);
        if (int rc = e_scan(ctx, d_hit, d_hits, n_oo)) return rc;
        if (int rc = flag_count(ctx, d_hit, d_hits, n_oo, &n_dup)) return rc;
        if (n_dup) {
          NTS_WS(d_dl, uint32_t*, "e_dup_l", n_dup * 4);
          NTS_WS(d_he, uint32_t*, "e_dup_e", n_dup * 4);
          NTS_WS(d_hw, uint32_t*, "e_dup_w", n_dup * 4);
          NTS_WS(d_di, uint32_t*, "e_dup_i", n_dup * 4);
          NTS_LAUNCH(k_e_take_flagged, E_GRID(n_oo), d_hit, d_hits, n_oo, q_idx, d_hedge, q_w, d_di, d_dl, d_he, d_hw);
          NTS_LAUNCH(k_e_set_u32, E_GRID(n_dup), E->e_w, d_he, d_hw, 0u, n_dup);
          // keep flags of the new edges: all but the duplicates
          HIP_TRY(ctx, hipMemsetAsync(d_oo, 0, lne * 8, ctx->stream));
          NTS_LAUNCH(k_e_not, E_GRID(lne), d_oo, lne);
          NTS_LAUNCH(k_e_zero64_at, E_GRID(n_dup), d_oo, d_dl, n_dup);
          if (int rc = e_scan(ctx, d_oo, d_oos, lne)) return rc;
        }
      }
    }
    if (int rc = e_reserve_edges(ctx, E, ne0 + lne - n_dup)) return rc;
    NTS_LAUNCH(k_e_append_edges, E_GRID(lne), n_dup ? d_oo : (const uint64_t*)nullptr, d_oos, lne, d_gu, d_gv, GD.e_w, ne0, E->e_u,
                       E->e_v, E->e_w, E->e_alive);
    E->ne = ne0 + lne - n_dup;
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (nv_out) *nv_out = E->nv;
  if (ne_out) *ne_out = E->ne;
  return NTS_OK;
}

// The sub-graph run_graph_simplification (S:566-590) looks at: candidate edges (both ends of degree 3) and every live edge
// incident to one of their end points, as host arrays owned by the library (nts_bubbles_free).
int nts_engine_bubbles(nts_ctx* ctx, nts_engine* E, nts_bubbles* out)
{
  if (!ctx || !E || !out) return fail(ctx, NTS_EINVAL, "nts_engine_bubbles: bad arguments");
  memset(out, 0, sizeof(*out));
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (E->ne == 0) return NTS_OK;
  uint32_t* d_deg = nullptr;
  if (int rc = e_degrees(ctx, E, &d_deg, nullptr, nullptr)) return rc;
  NTS_WS(d_cv, uint8_t*, "e_iscv", E->nv);
  NTS_WS(d_f, uint64_t*, "e_flag", std::max(E->ne, E->nv) * 8);
  NTS_WS(d_s, uint64_t*, "e_scan", std::max(E->ne, E->nv) * 8);
  HIP_TRY(ctx, hipMemsetAsync(d_cv, 0, E->nv, ctx->stream));
  NTS_LAUNCH(k_e_bubble_cand, E_GRID(E->ne), E->e_u, E->e_v, E->e_alive, E->ne, d_deg, d_cv, d_f);
  if (int rc = e_scan(ctx, d_f, d_s, E->ne)) return rc;
  uint64_t n_cand = 0;
  if (int rc = flag_count(ctx, d_f, d_s, E->ne, &n_cand)) return rc;
  if (n_cand == 0) return NTS_OK;
  NTS_WS(c_idx, uint32_t*, "e_c_idx", n_cand * 4);
  NTS_WS(c_u, uint32_t*, "e_c_u", n_cand * 4);
  NTS_WS(c_v, uint32_t*, "e_c_v", n_cand * 4);
  NTS_LAUNCH(k_e_take_flagged, E_GRID(E->ne), d_f, d_s, E->ne, E->e_u, E->e_v, (const uint32_t*)nullptr, c_idx, c_u, c_v, (uint32_t*)nullptr);
  out->n_cand = n_cand;
  out->cand_edge = host_copy(ctx, c_idx, n_cand);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  NTS_LAUNCH(k_e_incident, E_GRID(E->ne), E->e_u, E->e_v, E->e_alive, E->ne, d_cv, d_f);
  if (int rc = e_scan(ctx, d_f, d_s, E->ne)) return rc;
  uint64_t n_inc = 0;
  if (int rc = flag_count(ctx, d_f, d_s, E->ne, &n_inc)) return rc;
  NTS_WS(i_idx, uint32_t*, "e_i_idx", n_inc * 4);
  NTS_WS(i_u, uint32_t*, "e_i_u", n_inc * 4);
  NTS_WS(i_v, uint32_t*, "e_i_v", n_inc * 4);
  NTS_WS(i_w, uint32_t*, "e_i_w", n_inc * 4);
  NTS_LAUNCH(k_e_take_flagged, E_GRID(E->ne), d_f, d_s, E->ne, E->e_u, E->e_v, E->e_w, i_idx, i_u, i_v, i_w);
  out->n_inc = n_inc;
  out->inc_edge = host_copy(ctx, i_idx, n_inc);
  out->inc_u = host_copy(ctx, i_u, n_inc);
  out->inc_v = host_copy(ctx, i_v, n_inc);
  out->inc_w = host_copy(ctx, i_w, n_inc);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (!out->cand_edge || !out->inc_edge || !out->inc_u || !out->inc_v || !out->inc_w) {
    nts_bubbles_free(out);
    return fail(ctx, NTS_ENOMEM, "nts_engine_bubbles: host allocation failed");
  }
  return NTS_OK;
}

void nts_bubbles_free(nts_bubbles* b)
{
  if (!b) return;
  free(b->cand_edge);
  free(b->inc_edge);
  free(b->inc_u);
  free(b->inc_v);
  free(b->inc_w);
  memset(b, 0, sizeof(*b));
}

// Outcome of the simplification rule: the weight of `promote` edges becomes `weight` (S:586), `dead` vertices are deleted with
// their edges (S:589-590; the caller passes none in refinement rounds, where the reference loses the deletions, S:483-491).
int nts_engine_apply(nts_ctx* ctx, nts_engine* E, const uint32_t* dead, uint64_t n_dead, const uint32_t* promote, uint64_t n_promote,
                     uint32_t weight)
{
  if (!ctx || !E || (n_dead && !dead) || (n_promote && !promote)) return fail(ctx, NTS_EINVAL, "nts_engine_apply: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  for (uint64_t i = 0; i < n_dead; ++i)
    if (dead[i] >= E->nv) return fail(ctx, NTS_EINVAL, "nts_engine_apply: vertex out of range");
  for (uint64_t i = 0; i < n_promote; ++i)
    if (promote[i] >= E->ne) return fail(ctx, NTS_EINVAL, "nts_engine_apply: edge out of range");
  if (n_promote) {
    NTS_WS(d_p, uint32_t*, "e_apply_p", n_promote * 4);
    HIP_TRY(ctx, hipMemcpyAsync(d_p, promote, n_promote * 4, hipMemcpyHostToDevice, ctx->stream));
    NTS_LAUNCH(k_e_set_u32, E_GRID(n_promote), E->e_w, d_p, (const uint32_t*)nullptr, weight, n_promote);
  }
  if (n_dead) {
    NTS_WS(d_d, uint32_t*, "e_apply_d", n_dead * 4);
    NTS_WS(d_dead, uint8_t*, "e_dead", E->nv);
    HIP_TRY(ctx, hipMemcpyAsync(d_d, dead, n_dead * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_dead, 0, E->nv, ctx->stream));
    NTS_LAUNCH(k_e_set_u8, E_GRID(n_dead), d_dead, d_d, (uint8_t)1, n_dead);
    NTS_LAUNCH(k_e_kill, E_GRID(std::max(E->nv, E->ne)), d_dead, E->nv, E->v_alive, E->e_u, E->e_v, E->ne, E->e_alive);
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // the host arrays were read by asynchronous copies
  return NTS_OK;
}

// filter_graph_global (S:491, S:617): edges lighter than min_weight die; with `flag` they are remembered as (source, target)
// pairs for nts_engine_erode (filter_graph_global_flag_overlaps, S:292-303).
int nts_engine_filter(nts_ctx* ctx, nts_engine* E, uint32_t min_weight, int flag, uint64_t* n_light)
{
  if (!ctx || !E) return fail(ctx, NTS_EINVAL, "nts_engine_filter: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  E->n_flag = 0;
  if (n_light) *n_light = 0;
  if (E->ne == 0) return NTS_OK;
  NTS_WS(d_f, uint64_t*, "e_flag", std::max(E->ne, E->nv) * 8);
  NTS_WS(d_s, uint64_t*, "e_scan", std::max(E->ne, E->nv) * 8);
  NTS_LAUNCH(k_e_light, E_GRID(E->ne), E->e_w, E->e_alive, E->ne, min_weight, d_f);
  if (!flag && !n_light) return NTS_OK;
  if (int rc = e_scan(ctx, d_f, d_s, E->ne)) return rc;
  uint64_t n = 0;
  if (int rc = flag_count(ctx, d_f, d_s, E->ne, &n)) return rc;
  if (n_light) *n_light = n;
  if (flag && n) {
    if (n > E->cap_flag) {
      dev_free(E->fl_u);
      dev_free(E->fl_v);
      E->fl_u = E->fl_v = nullptr;
      E->cap_flag = 0;
      if (dev_malloc((void**)&E->fl_u, n * 4) != hipSuccess || dev_malloc((void**)&E->fl_v, n * 4) != hipSuccess)
        return fail(ctx, NTS_ENOMEM, "nts_engine_filter: hipMalloc");
      E->cap_flag = n;
    }
    NTS_WS(d_idx, uint32_t*, "e_fl_idx", n * 4);
    NTS_LAUNCH(k_e_take_flagged, E_GRID(E->ne), d_f, d_s, E->ne, E->e_u, E->e_v, (const uint32_t*)nullptr, d_idx, E->fl_u, E->fl_v,
                       (uint32_t*)nullptr);
    E->n_flag = n;
  }
  HIP_TRY(ctx, hipGetLastError());
  return NTS_OK;
}

// refine_graph + erode_edges (S:305-362) over the pairs flagged by the last nts_engine_filter(flag = 1)
int nts_engine_erode(nts_ctx* ctx, nts_engine* E, uint32_t k, uint64_t* n_dead_edges)
{
  if (!ctx || !E) return fail(ctx, NTS_EINVAL, "nts_engine_erode: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (n_dead_edges) *n_dead_edges = 0;
  if (E->n_flag == 0 || E->ne == 0) return NTS_OK;
  uint32_t *d_deg = nullptr, *d_nbr = nullptr, *d_nbe = nullptr;
  if (int rc = e_degrees(ctx, E, &d_deg, &d_nbr, &d_nbe)) return rc;
  NTS_WS(d_edead, uint8_t*, "e_edead", E->ne);
  NTS_WS(d_ctl, unsigned long long*, "e_ctl", 64);
  NTS_WS(d_later, uint32_t*, "e_later", E->n_flag * 4);
  HIP_TRY(ctx, hipMemsetAsync(d_edead, 0, E->ne, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(d_ctl, 0, 64, ctx->stream));
  const uint32_t all_later = NTS_KNOB("NTS_ERODE_HOST") && atoi(NTS_KNOB("NTS_ERODE_HOST")) ? 1u : 0u; // (tests: every pair on the host)
  NTS_LAUNCH(k_e_erode, E_GRID(E->n_flag), E->fl_u, E->fl_v, E->n_flag, E->v_hash, E->v_pos, E->cap_v, E->G, d_deg, d_nbr, d_nbe,
                     (uint64_t)k, d_edead, d_later, d_ctl + 1, all_later);
  unsigned long long n_later = 0;
  if (int rc = e_fetch(ctx, d_ctl + 1, &n_later, 1)) return rc;
  if (n_later) {
    // The pairs the kernel left: the same walk on the host, over every live edge of a vertex (a vertex on the walk may have
    // more than two -- the reference only asks that exactly one of its neighbours is new, S:329-331).  Rare; the graph comes
    // down once, a vertex's edges are found by a scan.
    const uint64_t ne = E->ne, nv = E->nv;
    std::vector<uint32_t> eu(ne), ev(ne), flu(E->n_flag), flv(E->n_flag), later(n_later);
    std::vector<uint8_t> alive(ne);
    std::vector<uint64_t> vh(nv), vpos((size_t)E->G * nv);
    HIP_TRY(ctx, hipMemcpyAsync(eu.data(), E->e_u, ne * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ev.data(), E->e_v, ne * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(alive.data(), E->e_alive, ne, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(flu.data(), E->fl_u, E->n_flag * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(flv.data(), E->fl_v, E->n_flag * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(later.data(), d_later, n_later * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(vh.data(), E->v_hash, nv * 8, hipMemcpyDeviceToHost, ctx->stream));
    for (uint32_t g = 0; g < E->G; ++g)
      HIP_TRY(ctx, hipMemcpyAsync(vpos.data() + (size_t)g * nv, E->v_pos + (uint64_t)g * E->cap_v, nv * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::map<uint32_t, std::vector<std::pair<uint64_t, uint32_t>>> inc; // vertex -> (edge, other end) over the live edges
    // a handful of pairs: a vertex's edges by a scan of the edge list; more than that: the adjacency of the whole graph, once (a scan per
    // vertex of a walk is ne steps each -- thousands of left-over pairs on a graph of 10^8 edges would be hours)
    std::vector<uint64_t> adj_off;
    std::vector<uint32_t> adj_e;
    if (later.size() > 8) {
      adj_off.assign(nv + 1, 0);
      for (uint64_t e = 0; e < ne; ++e)
        if (alive[e]) {
          ++adj_off[eu[e] + 1];
          ++adj_off[ev[e] + 1];
        }
      for (uint64_t v = 0; v < nv; ++v) adj_off[v + 1] += adj_off[v];
      adj_e.resize(adj_off[nv]);
      std::vector<uint64_t> at(adj_off.begin(), adj_off.end() - 1);
      for (uint64_t e = 0; e < ne; ++e) // (ascending edge order per vertex, as the scan below yields it)
        if (alive[e]) {
          adj_e[at[eu[e]]++] = (uint32_t)e;
          adj_e[at[ev[e]]++] = (uint32_t)e;
        }
    }
    auto neighbours = [&](uint32_t v) -> const std::vector<std::pair<uint64_t, uint32_t>>& {
      auto it = inc.find(v);
      if (it != inc.end()) return it->second;
      auto& out = inc[v];
      if (!adj_off.empty()) {
        for (uint64_t q = adj_off[v]; q < adj_off[v + 1]; ++q) {
          const uint64_t e = adj_e[q];
          if (eu[e] == v && ev[e] == v && !out.empty() && out.back().first == e) continue; // (a loop is listed once)
          out.emplace_back(e, eu[e] == v ? ev[e] : eu[e]);
        }
        return out;
      }
      for (uint64_t e = 0; e < ne; ++e)
        if (alive[e] && (eu[e] == v || ev[e] == v)) out.emplace_back(e, eu[e] == v ? ev[e] : eu[e]);
      return out;
    };
    auto too_close = [&](uint32_t a, uint32_t b) {
      for (uint32_t g = 0; g < E->G; ++g) {
        const uint64_t pa = vpos[(size_t)g * nv + a], pb = vpos[(size_t)g * nv + b];
        if ((pa > pb ? pa - pb : pb - pa) < k) return true;
      }
      return false;
    };
    std::vector<uint64_t> dead;
    for (uint32_t i : later) {
      uint32_t s = flu[i], t = flv[i];
      if (std::to_string(vh[s]) > std::to_string(vh[t])) std::swap(s, t); // decimal strings (S:351)
      if (neighbours(s).size() != 1 || neighbours(t).size() != 1) continue;
      std::set<uint32_t> visited{ s, t };
      bool erode_target = true;
      uint32_t cs = s, ct = t;
      while (too_close(cs, ct)) {
        const uint32_t v = erode_target ? ct : cs;
        uint32_t nxt = E_NONE;
        int n_nxt = 0;
        for (const auto& en : neighbours(v)) {
          dead.push_back(en.first);
          if (!visited.count(en.second)) {
            nxt = en.second;
            ++n_nxt;
          }
        }
        if (n_nxt == 0) break;
        if (n_nxt > 1)
          return fail(ctx, NTS_ERANGE, "nts_engine_erode: the erosion walk has two ways on at a vertex (the reference's assert at bin/ntsynt_synteny.py:330)");
        (erode_target ? ct : cs) = nxt;
        visited.insert(nxt);
        erode_target = !erode_target;
      }
    }
    if (!dead.empty()) {
      NTS_WS(d_didx, uint64_t*, "e_later_dead", dead.size() * 8);
      HIP_TRY(ctx, hipMemcpyAsync(d_didx, dead.data(), dead.size() * 8, hipMemcpyHostToDevice, ctx->stream));
      NTS_LAUNCH(k_e_mark_u8, E_GRID(dead.size()), d_didx, dead.size(), d_edead);
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // (`dead` leaves scope)
    }
  }
  NTS_LAUNCH(k_e_apply_dead_edges, E_GRID(E->ne), d_edead, E->e_alive, E->ne, d_ctl);
  unsigned long long n_dead = 0;
  if (int rc = e_fetch(ctx, d_ctl, &n_dead, 1)) return rc;
  if (n_dead_edges) *n_dead_edges = n_dead;
  return NTS_OK;
}

// Paths of the graph and their synteny blocks (rows C5-C9).  bp: indel threshold (S:364-409); m_percent: orientation
// threshold (synteny_block.py:48-65); min_mx: filter_synteny_blocks' minimum (4 in the reference).  The vertices of paths
// without an orientation and of blocks below min_mx are deleted, edges at indel cuts die, and the kept blocks' end /
// interior vertices are marked for the next refinement round's nts_engine_add.
int nts_engine_blocks(nts_ctx* ctx, nts_engine* E, int64_t bp, double m_percent, uint32_t min_mx, nts_blocks* out)
{
  if (!ctx || !E || !out) return fail(ctx, NTS_EINVAL, "nts_engine_blocks: bad arguments");
  memset(out, 0, sizeof(*out));
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const bool trace = NTS_KNOB("NTS_HOST_DEBUG") != nullptr;
  auto t_last = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (!trace) return;
    hipStreamSynchronize(ctx->stream);
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "nts_engine_blocks %-14s %.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
    t_last = now;
  };
  E->n_paths = E->n_path_verts = 0;
  const uint64_t nv = E->nv, G = E->G;
  if (nv == 0) return NTS_OK;
  HIP_TRY(ctx, hipMemsetAsync(E->internal, 0, nv, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(E->terminal, 0, nv, ctx->stream));
  uint32_t *d_deg = nullptr, *d_nbr = nullptr, *d_nbe = nullptr;
  if (int rc = e_degrees(ctx, E, &d_deg, &d_nbr, &d_nbe)) return rc;
  lap("degrees");
  // ---- list ranking
  NTS_WS(d_st0, uint4*, "e_arc0", 2 * nv * 16);
  NTS_WS(d_st1, uint4*, "e_arc1", 2 * nv * 16);
  NTS_LAUNCH(k_e_arc_init, E_GRID(2 * nv), d_deg, d_nbr, nv, d_st0);
  int rounds = 1;
  while (((uint64_t)1 << rounds) < nv + 1) ++rounds;
  rounds += 1;
  uint4 *a = d_st0, *b = d_st1;
  {
    ScopedTimer t(ctx, "list_ranking");
    for (int r = 0; r < rounds; ++r) {
      NTS_LAUNCH(k_e_arc_jump, E_GRID(2 * nv), a, b, 2 * nv);
      std::swap(a, b);
    }
  }
  lap("pointer jumps");
  NTS_WS(d_pstart, uint32_t*, "e_pstart", nv * 4);
  NTS_WS(d_pidx, uint32_t*, "e_pidx", nv * 4);
  NTS_WS(d_plen, uint32_t*, "e_plen", nv * 4);
  NTS_WS(d_f, uint64_t*, "e_flag", std::max(E->ne, nv) * 8);
  NTS_WS(d_s, uint64_t*, "e_scan", std::max(E->ne, nv) * 8);
  NTS_LAUNCH(k_e_classify, E_GRID(nv), d_deg, a, nv, E->v_pos + (uint64_t)E->ref * E->cap_v, d_pstart, d_pidx, d_plen, d_f);
  if (int rc = e_scan(ctx, d_f, d_s, nv)) return rc;
  uint64_t n_paths = 0;
  if (int rc = flag_count(ctx, d_f, d_s, nv, &n_paths)) return rc;
  out->stats_paths = n_paths;
  if (n_paths == 0) return NTS_OK;
  NTS_WS(d_lens, uint64_t*, "e_lens", (n_paths + 1) * 8);
  NTS_WS(d_poff, uint64_t*, "e_poff", (n_paths + 1) * 8);
  HIP_TRY(ctx, hipMemsetAsync(d_lens + n_paths, 0, 8, ctx->stream));
  NTS_LAUNCH(k_e_path_len, E_GRID(nv), d_f, d_s, d_plen, nv, d_lens);
  if (int rc = e_scan(ctx, d_lens, d_poff, n_paths + 1)) return rc;
  uint64_t N = 0;
  if (int rc = e_fetch(ctx, d_poff + n_paths, &N)) return rc;
  NTS_WS(d_verts, uint32_t*, "e_verts", (N + 1) * 4);
  NTS_WS(d_vpath, uint32_t*, "e_vpath", N * 4);
  NTS_LAUNCH(k_e_place, E_GRID(nv), d_pstart, d_pidx, d_s, d_poff, nv, d_verts, d_vpath);
  E->n_paths = n_paths;
  E->n_path_verts = N;
  lap("path order");
  // ---- per-path scan
  NTS_WS(d_pst, uint32_t*, "e_pst", n_paths * 4);
  NTS_WS(d_nup, uint32_t*, "e_nup", G * n_paths * 4);
  NTS_WS(d_over, uint8_t*, "e_over", N + 1);
  NTS_WS(d_pcode, uint8_t*, "e_pcode", G * n_paths);
  NTS_WS(d_pgood, uint8_t*, "e_pgood", n_paths);
  NTS_WS(d_ctl, unsigned long long*, "e_ctl", 64);
  NTS_WS(d_dead, uint8_t*, "e_dead", nv);
  HIP_TRY(ctx, hipMemsetAsync(d_nup, 0, G * n_paths * 4, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(d_ctl, 0, 64, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(d_dead, 0, nv, ctx->stream));
  NTS_LAUNCH(k_e_run_init, E_GRID(n_paths), d_poff, n_paths, d_pst);
  NTS_LAUNCH(k_e_run_start, E_GRID(N), d_verts, d_vpath, N, d_poff, E->v_rec, E->cap_v, E->G, d_pst);
  NTS_LAUNCH(k_e_steps, E_GRID(N), d_verts, d_vpath, N, d_poff, d_pst, E->v_pos, E->cap_v, E->G, n_paths, bp, d_nup, d_over);
  NTS_LAUNCH(k_e_orient, E_GRID(n_paths), d_poff, d_pst, d_nup, n_paths, E->G, m_percent, d_pcode, d_pgood, d_ctl);
  lap("path scans");
  // ---- blocks
  NTS_WS(d_bs, uint64_t*, "e_bstart", N * 8);
  NTS_WS(d_bscan, uint64_t*, "e_bscan", N * 8);
  NTS_LAUNCH(k_e_block_starts, E_GRID(N), d_verts, d_vpath, N, d_poff, d_pst, d_pgood, d_over, d_dead, d_bs);
  NTS_LAUNCH(k_e_cuts, E_GRID(N), d_verts, N, d_over, d_nbr, d_nbe, E->e_alive, d_ctl + 1);
  if (int rc = e_scan(ctx, d_bs, d_bscan, N)) return rc;
  uint64_t n_blocks = 0;
  if (int rc = flag_count(ctx, d_bs, d_bscan, N, &n_blocks)) return rc;
  uint64_t n_kept = 0;
  uint64_t *d_bkeep = nullptr, *d_bwhere = nullptr;
  uint32_t *d_bfirst = nullptr, *d_blast = nullptr, *d_bpath = nullptr;
  if (n_blocks) {
    d_bfirst = (uint32_t*)ws_get(ctx, "e_bfirst", n_blocks * 4);
    d_blast = (uint32_t*)ws_get(ctx, "e_blast", n_blocks * 4);
    d_bpath = (uint32_t*)ws_get(ctx, "e_bpath", n_blocks * 4);
    d_bkeep = (uint64_t*)ws_get(ctx, "e_bkeep", n_blocks * 8);
    d_bwhere = (uint64_t*)ws_get(ctx, "e_bwhere", n_blocks * 8);
    if (!d_bfirst || !d_blast || !d_bpath || !d_bkeep || !d_bwhere) return NTS_ENOMEM;
    NTS_LAUNCH(k_e_block_bounds, E_GRID(N), d_vpath, N, d_poff, d_pst, d_pgood, d_over, d_bs, d_bscan, d_bfirst, d_blast, d_bpath);
    NTS_LAUNCH(k_e_block_keep, E_GRID(n_blocks), d_bfirst, d_blast, n_blocks, min_mx, d_bkeep, d_ctl + 2);
    NTS_LAUNCH(k_e_block_marks, E_GRID(N), d_verts, d_vpath, N, d_pst, d_pgood, d_bs, d_bscan, d_bkeep, d_bfirst, d_blast, d_dead,
                       E->internal, E->terminal);
    if (int rc = e_scan(ctx, d_bkeep, d_bwhere, n_blocks)) return rc;
    if (int rc = flag_count(ctx, d_bkeep, d_bwhere, n_blocks, &n_kept)) return rc;
  }
  NTS_LAUNCH(k_e_kill, E_GRID(std::max(nv, E->ne)), d_dead, nv, E->v_alive, E->e_u, E->e_v, E->ne, E->e_alive);
  unsigned long long ctl[3] = { 0, 0, 0 };
  if (int rc = e_fetch(ctx, d_ctl, ctl, 3)) return rc;
  lap("block rules");
  out->stats_unoriented = ctl[0];
  out->stats_indel_cuts = ctl[1];
  out->stats_small = ctl[2];
  out->n_blocks = n_kept;
  if (n_kept == 0) return NTS_OK;
  NTS_WS(o_first, uint32_t*, "e_o_first", n_kept * 4);
  NTS_WS(o_last, uint32_t*, "e_o_last", n_kept * 4);
  NTS_WS(o_n, uint32_t*, "e_o_n", n_kept * 4);
  NTS_WS(o_rec, uint32_t*, "e_o_rec", G * n_kept * 4);
  NTS_WS(o_fp, uint64_t*, "e_o_fp", G * n_kept * 8);
  NTS_WS(o_lp, uint64_t*, "e_o_lp", G * n_kept * 8);
  NTS_WS(o_ori, uint8_t*, "e_o_ori", G * n_kept);
  NTS_LAUNCH(k_e_block_table, E_GRID(n_blocks), d_bkeep, d_bwhere, n_blocks, n_kept, d_bfirst, d_blast, d_bpath, d_verts, d_pst, d_pcode,
                     n_paths, E->v_rec, E->v_pos, E->cap_v, E->G, o_first, o_last, o_n, o_rec, o_fp, o_lp, o_ori);
  HIP_TRY(ctx, hipGetLastError());
  out->first_vid = host_copy(ctx, o_first, n_kept);
  out->last_vid = host_copy(ctx, o_last, n_kept);
  out->n_mx = host_copy(ctx, o_n, n_kept);
  out->rec = host_copy(ctx, o_rec, G * n_kept);
  out->first_pos = host_copy(ctx, o_fp, G * n_kept);
  out->last_pos = host_copy(ctx, o_lp, G * n_kept);
  out->ori = host_copy(ctx, o_ori, G * n_kept);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (!out->first_vid || !out->last_vid || !out->n_mx || !out->rec || !out->first_pos || !out->last_pos || !out->ori) {
    nts_blocks_free(out);
    return fail(ctx, NTS_ENOMEM, "nts_engine_blocks: host allocation failed");
  }
  return NTS_OK;
}

// A list sketched from a batch genome (nts_genome_concat) taken apart on the device: part p = the minimizers of records
// [rec_base[p], rec_base[p+1]), record ids rebased to the part.  The list is in (record, position) order, so each part is a
// slice; nothing visits the host but the n_parts + 1 slice bounds.
int nts_mx_split(nts_ctx* ctx, const nts_mx* mx, uint32_t n_parts, const uint32_t* rec_base, nts_mx** out)
{
  if (!ctx || !mx || !out || n_parts == 0 || !rec_base) return fail(ctx, NTS_EINVAL, "nts_mx_split: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  for (uint32_t p = 0; p < n_parts; ++p) out[p] = nullptr;
  std::vector<uint64_t> cut(n_parts + 1, 0);
  if (mx->n) {
    uint32_t* d_base = (uint32_t*)ws_get(ctx, "split_base", (n_parts + 1) * 4);
    uint64_t* d_cut = (uint64_t*)ws_get(ctx, "split_cut", (n_parts + 1) * 8);
    if (!d_base || !d_cut) return NTS_ENOMEM;
    HIP_TRY(ctx, hipMemcpyAsync(d_base, rec_base, (n_parts + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    NTS_LAUNCH(k_e_rec_bounds, dim3(1), dim3(256), 0, ctx->stream, mx->d_rec, mx->n, d_base, n_parts + 1, d_cut);
    HIP_TRY(ctx, hipMemcpyAsync(cut.data(), d_cut, (n_parts + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  for (uint32_t p = 0; p < n_parts; ++p) {
    const uint64_t a = cut[p], b = cut[p + 1], n = b > a ? b - a : 0;
    nts_mx* part = new nts_mx();
    part->n = n;
    out[p] = part;
    if (!n) continue;
    if (dev_malloc((void**)&part->d_h1, n * 20) != hipSuccess) {
      for (uint32_t q = 0; q <= p; ++q) nts_mx_free(ctx, out[q]), out[q] = nullptr;
      return fail(ctx, NTS_ENOMEM, "nts_mx_split: hipMalloc");
    }
    part->cap_bytes = n * 20;
    part->d_pos = part->d_h1 + n;
    part->d_rec = (uint32_t*)(part->d_pos + n);
    hipMemcpyAsync(part->d_h1, mx->d_h1 + a, n * 8, hipMemcpyDeviceToDevice, ctx->stream);
    hipMemcpyAsync(part->d_pos, mx->d_pos + a, n * 8, hipMemcpyDeviceToDevice, ctx->stream);
    NTS_LAUNCH(k_e_rebase, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, mx->d_rec + a, n, rec_base[p], part->d_rec);
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return NTS_OK;
}

// The lists of a genome's shards (nts_genome_slice; in record order) as the genome's list: part p's record numbers are raised by
// rec_offset[p].  The inverse of nts_mx_split.
int nts_mx_concat(nts_ctx* ctx, uint32_t n_parts, const nts_mx* const* parts, const uint32_t* rec_offset, nts_mx** out)
{
  if (!ctx || !out || n_parts == 0 || !parts || !rec_offset) return fail(ctx, NTS_EINVAL, "nts_mx_concat: bad arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  uint64_t n = 0;
  for (uint32_t p = 0; p < n_parts; ++p) {
    if (!parts[p]) return fail(ctx, NTS_EINVAL, "nts_mx_concat: NULL part");
    n += parts[p]->n;
  }
  nts_mx* mx = new nts_mx();
  mx->n = n;
  *out = mx;
  if (!n) return NTS_OK;
  if (alloc_result(ctx, mx, n) != NTS_OK) {
    delete mx;
    *out = nullptr;
    return fail(ctx, NTS_ENOMEM, "nts_mx_concat: hipMalloc");
  }
  uint64_t at = 0;
  for (uint32_t p = 0; p < n_parts; ++p) {
    const uint64_t m = parts[p]->n;
    if (!m) continue;
    hipMemcpyAsync(mx->d_h1 + at, parts[p]->d_h1, m * 8, hipMemcpyDeviceToDevice, ctx->stream);
    hipMemcpyAsync(mx->d_pos + at, parts[p]->d_pos, m * 8, hipMemcpyDeviceToDevice, ctx->stream);
    // (k_e_rebase subtracts its base: the two's complement of the offset adds it)
    NTS_LAUNCH(k_e_rebase, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, ctx->stream, parts[p]->d_rec, m, 0u - rec_offset[p], mx->d_rec + at);
    at += m;
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return NTS_OK;
}

int nts_mx_screen(nts_ctx* ctx, const nts_genome* g, const nts_mx* mx, uint32_t k, const nts_bf* filter_out, nts_mx** out)
{
  if (!ctx || !g || !mx || !filter_out || !out || k == 0) return fail(ctx, NTS_EINVAL, "nts_mx_screen: bad arguments");
  if (!g->d_code || !g->d_rec_off) return fail(ctx, NTS_EINVAL, "nts_mx_screen: the genome's bases are not resident");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  *out = nullptr;
  nts_mx* res = new nts_mx();
  const uint64_t n = mx->n;
  uint64_t kept = 0;
  uint32_t* d_keep = nullptr;
  uint64_t* d_at = nullptr;
  if (n) {
    d_keep = (uint32_t*)ws_get(ctx, "screen_keep", n * 4);
    d_at = (uint64_t*)ws_get(ctx, "screen_at", n * 8);
    if (!d_keep || !d_at) {
      delete res;
      return NTS_ENOMEM;
    }
    const HashParams hp = make_hash_params(k);
    NTS_LAUNCH(k_mx_screen_flags, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, g->d_code + PAD, g->d_rec_off, mx->d_rec, mx->d_pos, n, hp,
                       filter_out->d_words, make_fastmod(filter_out->bytes * 8), d_keep);
    if (int rc = scan_counts<uint32_t>(ctx, d_keep, n, d_at)) {
      delete res;
      return rc;
    }
    uint64_t last_at = 0;
    uint32_t last_keep = 0;
    hipMemcpyAsync(&last_at, d_at + (n - 1), 8, hipMemcpyDeviceToHost, ctx->stream);
    hipMemcpyAsync(&last_keep, d_keep + (n - 1), 4, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
      delete res;
      return fail(ctx, NTS_EHIP, std::string("nts_mx_screen: ") + hipGetErrorString(e));
    }
    kept = last_at + last_keep;
  }
  res->n = kept;
  if (kept) {
    if (alloc_result(ctx, res, kept) != NTS_OK) {
      delete res;
      return fail(ctx, NTS_ENOMEM, "nts_mx_screen: hipMalloc");
    }
    NTS_LAUNCH(k_mx_screen_move, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, mx->d_h1, mx->d_rec, mx->d_pos, d_keep, d_at, n, res->d_h1,
                       res->d_rec, res->d_pos);
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
      nts_mx_free(ctx, res);
      return fail(ctx, NTS_EHIP, std::string("nts_mx_screen: ") + hipGetErrorString(e));
    }
  }
  *out = res;
  return NTS_OK;
}

void nts_blocks_free(nts_blocks* b)
{
  if (!b) return;
  free(b->first_vid);
  free(b->last_vid);
  free(b->n_mx);
  free(b->rec);
  free(b->first_pos);
  free(b->last_pos);
  free(b->ori);
  memset(b, 0, sizeof(*b));
}

} // extern "C"

#undef E_GRID

// nts_fasta_dev.inc -- FASTA ingest with the parse on the GPU (SURVEY.md 8(f) rank 2), included by ntsynt_hip.hip.
//
// replaces btllib::SeqReader(path, LONG_MODE) record streaming (src/ntsynt_make_common_bf.cpp:32-36,125-131) and rule faidx
// (bin/ntsynt_run_pipeline.smk:48-53) without a host pass over the bases: the file's bytes (mapped, or inflated for .gz) go to
// HBM through pinned staging on a few host threads, and kernels find the header lines, drop line ends, compact and encode
// the bases into the resident genome, and produce the record table and the `samtools faidx` columns.  The host only reads the
// header lines themselves (record ids).  Same parsing rules as nts_fasta_read (csrc/nts_hostio.cpp), which stays as the
// host-side statement the tests compare with.  White space in sequence lines: carriage returns are dropped wherever they are;
// blanks, tabs, vertical tabs and form feeds that run up to the start or the end of their line are dropped (the reference's
// SeqReader trims its lines -- recalled, btllib is not in the tree; the oracle's reader strips both ends); anywhere else they
// stay as invalid bases, as any other byte that is not a nucleotide.
extern "C" int nts_internal_file_open(const char* path, const uint8_t** p, uint64_t* n, void** handle);
extern "C" void nts_internal_file_close(void* handle);

namespace {

constexpr uint32_t FA_TILE = 16384; // raw bytes per workgroup (256 lanes x 64)
constexpr uint64_t FA_NONE = ~0ULL;

// last header r with hdr_start[r] <= i, or -1
__device__ __forceinline__ int64_t fa_header_before(const uint64_t* __restrict__ hs, uint64_t n_hdr, uint64_t i)
{
  uint64_t lo = 0, hi = n_hdr;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (hs[mid] <= i)
      lo = mid + 1;
    else
      hi = mid;
  }
  return (int64_t)lo - 1;
}

// A whole tile of the file image (FA_TILE bytes, 16-byte aligned) into LDS with coalesced 16-byte loads, laid out so that every
// lane then reads its own 64 consecutive bytes as sixteen words without bank conflicts (a lane's chunk every 17 words).  The
// kernels below used to read their 64 bytes one byte at a time from global memory, lanes 64 bytes apart -- every load
// instruction touched 64 lines: 7 + 8 + 13 ms per 3 GB file, 0.4 TB/s.
constexpr uint32_t FA_LSTRIDE = 17;

__device__ __forceinline__ void fa_stage_tile(const uint8_t* __restrict__ raw, uint64_t tile_base, uint32_t* s_raw, uint32_t (&dw)[16])
{
  const uint4* src = reinterpret_cast<const uint4*>(raw + tile_base);
  uint4 v[4];
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) v[q] = src[q * 256u + threadIdx.x];
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {
    const uint32_t idx = q * 256u + threadIdx.x;
    uint32_t* d = s_raw + (idx >> 2) * FA_LSTRIDE + (idx & 3u) * 4u;
    d[0] = v[q].x;
    d[1] = v[q].y;
    d[2] = v[q].z;
    d[3] = v[q].w;
  }
  __syncthreads();
#pragma unroll
  for (uint32_t w = 0; w < 16; ++w) dw[w] = s_raw[threadIdx.x * FA_LSTRIDE + w];
}

// 0x80 in every byte of x that equals c (exact per byte: no carries between bytes)
__device__ __forceinline__ uint32_t fa_bytes_eq(uint32_t x, uint32_t c)
{
  const uint32_t z = x ^ (c * 0x01010101u);
  return ~(((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z) & 0x80808080u;
}

// 0x80 in every byte of x below 0x21 (line ends, blanks, control characters)
__device__ __forceinline__ uint32_t fa_bytes_ctl(uint32_t x)
{
  return ~(((x & 0x7F7F7F7Fu) + 0x5F5F5F5Fu) | x) & 0x80808080u;
}

// header starts ('>' at the start of a line) and, per tile, the position of its first line feed
__global__ __launch_bounds__(256) void k_fa_scan(const uint8_t* __restrict__ raw, uint64_t n, uint64_t* __restrict__ hdr, uint64_t hdr_cap,
                                                 unsigned long long* __restrict__ n_hdr, uint64_t* __restrict__ tile_nl)
{
  __shared__ unsigned long long s_first;
  __shared__ uint32_t s_raw[256 * FA_LSTRIDE];
  if (threadIdx.x == 0) s_first = FA_NONE;
  __syncthreads();
  const uint64_t tile_base = (uint64_t)blockIdx.x * FA_TILE;
  const uint64_t base = tile_base + (uint64_t)threadIdx.x * 64;
  unsigned long long first = FA_NONE;
  if (tile_base + FA_TILE <= n) { // (uniform) a whole tile: bytes in registers, line feeds and '>' found four bytes at a time
    uint32_t dw[16];
    fa_stage_tile(raw, tile_base, s_raw, dw);
    uint32_t prev_word = threadIdx.x ? s_raw[(threadIdx.x - 1u) * FA_LSTRIDE + 15u] : ((tile_base ? (uint32_t)raw[tile_base - 1] : (uint32_t)'\n') << 24);
#pragma unroll
    for (uint32_t w = 0; w < 16; ++w) {
      const uint32_t nl = fa_bytes_eq(dw[w], '\n'), gt = fa_bytes_eq(dw[w], '>');
      if (nl && first == FA_NONE) first = base + 4u * w + ((uint32_t)__ffs((int)nl) - 1u) / 8u;
      if (gt) { // (rare) a header starts here if the byte before is a line feed
#pragma unroll
        for (uint32_t b = 0; b < 4; ++b)
          if ((gt >> (8u * b + 7u)) & 1u) {
            const uint32_t before = b ? (dw[w] >> (8u * (b - 1u))) & 0xFFu : prev_word >> 24;
            if (before == (uint32_t)'\n') {
              const unsigned long long at = atomicAdd(n_hdr, 1ull);
              if (at < hdr_cap) hdr[at] = base + 4u * w + b;
            }
          }
      }
      prev_word = dw[w];
    }
  } else if (base < n) {
    const uint64_t end = min(base + 64, n);
    uint8_t prev = base ? raw[base - 1] : (uint8_t)'\n';
    for (uint64_t i = base; i < end; ++i) {
      const uint8_t c = raw[i];
      if (c == '\n' && first == FA_NONE) first = i;
      if (c == '>' && prev == '\n') {
        const unsigned long long at = atomicAdd(n_hdr, 1ull);
        if (at < hdr_cap) hdr[at] = i;
      }
      prev = c;
    }
  }
  if (first != FA_NONE) atomicMin(&s_first, first);
  __syncthreads();
  if (threadIdx.x == 0) tile_nl[blockIdx.x] = s_first;
}

// first line feed at or after `from` (n if none): the rest of from's tile, then the per-tile table
__device__ uint64_t fa_find_nl(const uint8_t* __restrict__ raw, uint64_t n, const uint64_t* __restrict__ tile_nl, uint64_t n_tiles, uint64_t from,
                               unsigned long long* s_min)
{
  if (threadIdx.x == 0) *s_min = FA_NONE;
  __syncthreads();
  if (from >= n) return n;
  const uint64_t t0 = from / FA_TILE;
  const uint64_t t_end = min((t0 + 1) * FA_TILE, n);
  unsigned long long best = FA_NONE;
  for (uint64_t i = from + threadIdx.x; i < t_end; i += blockDim.x)
    if (raw[i] == '\n') {
      best = i;
      break;
    }
  if (best != FA_NONE) atomicMin(s_min, best);
  __syncthreads();
  unsigned long long got = *s_min;
  __syncthreads();
  if (got != FA_NONE) return got;
  // later tiles: the first tile holding a line feed
  for (uint64_t t = t0 + 1 + threadIdx.x; t < n_tiles; t += blockDim.x)
    if (tile_nl[t] != FA_NONE) {
      atomicMin(s_min, (unsigned long long)tile_nl[t]);
      break;
    }
  __syncthreads();
  got = *s_min;
  __syncthreads();
  return got == FA_NONE ? n : got;
}

// per header (one workgroup): end of the header line, and the first sequence line's extent for the faidx columns
__global__ __launch_bounds__(256) void k_fa_headers(const uint8_t* __restrict__ raw, uint64_t n, const uint64_t* __restrict__ hdr_start,
                                                    uint64_t n_hdr, const uint64_t* __restrict__ tile_nl, uint64_t n_tiles,
                                                    uint64_t* __restrict__ hdr_end, uint64_t* __restrict__ line_end)
{
  __shared__ unsigned long long s_min;
  const uint64_t r = blockIdx.x;
  const uint64_t he = fa_find_nl(raw, n, tile_nl, n_tiles, hdr_start[r], &s_min);
  const uint64_t le = fa_find_nl(raw, n, tile_nl, n_tiles, he + 1, &s_min);
  if (threadIdx.x == 0) {
    hdr_end[r] = he;
    line_end[r] = le;
  }
}

__device__ __forceinline__ bool fa_is_blank(uint8_t c) { return c == ' ' || c == '\t' || c == '\v' || c == '\f' || c == '\r'; }

// is byte i a base?  (not a line end, not inside a header line, not before the first header, not white space at either end of
// its line)
__device__ __forceinline__ bool fa_is_base(const uint8_t* __restrict__ raw, uint64_t n, uint64_t i, const uint64_t* __restrict__ hs,
                                           const uint64_t* __restrict__ he, int64_t& r, uint64_t n_hdr)
{
  while ((uint64_t)(r + 1) < n_hdr && hs[r + 1] <= i) ++r;
  if (r < 0 || i <= he[r]) return false;
  const uint8_t c = raw[i];
  if (c == '\n' || c == '\r') return false;
  if (fa_is_blank(c)) { // (rare) trailing: only white space up to the line end; leading: only white space back to the line start
    // Every blank byte walks its own run, so the walks are bounded: a run of more than FA_BLANK_SCAN blanks (a malformed or
    // hostile file -- 100 MB of spaces would cost run^2 loads) is not looked at as a whole; its bytes farther than that from
    // either line end count as bases (invalid ones: code 4), like white space in the middle of a line does.  A byte goes if
    // FEWER than FA_BLANK_SCAN blanks lie between it and the line's end (line feed or end of file), or its start: a trailing run
    // of b blanks keeps its first max(0, b - 4096), a leading run of a its last max(0, a - 4096), an all-blank line of L bytes
    // max(0, L - 8192).  (The host reader trims runs of any length: the one difference, tests/test_gpu_fasta_seams.py.)
    constexpr uint64_t FA_BLANK_SCAN = 4096;
    uint64_t q = i + 1;
    const uint64_t fwd_end = (n - i > FA_BLANK_SCAN) ? i + FA_BLANK_SCAN : n; // (fwd_end < n, or fwd_end == n == q below)
    while (q < fwd_end && fa_is_blank(raw[q])) ++q;
    if (q == n || raw[q] == '\n') return false; // the line feed may stand at fwd_end itself: FA_BLANK_SCAN - 1 blanks between
    q = i;
    const uint64_t back_end = (i > FA_BLANK_SCAN) ? i - FA_BLANK_SCAN : 0;
    while (q > back_end && fa_is_blank(raw[q - 1])) --q;
    if (q == 0 || (q > back_end && raw[q - 1] == '\n')) return false;
  }
  return true;
}

__device__ __forceinline__ uint8_t fa_code(uint8_t c)
{
  c &= 0xDFu; // fold case
  return (c == 'A') ? 0 : (c == 'C') ? 1 : (c == 'G') ? 2 : (c == 'T' || c == 'U') ? 3 : 4;
}

// PASS 0: bases per tile.  PASS 1: the tile's bases, encoded, to their place in the genome (staged in LDS, written out in
// runs of consecutive bytes).
template <int PASS>
__global__ __launch_bounds__(256) void k_fa_bases(const uint8_t* __restrict__ raw, uint64_t n, const uint64_t* __restrict__ hs,
                                                  const uint64_t* __restrict__ he, uint64_t n_hdr, uint64_t* __restrict__ tile_cnt,
                                                  const uint64_t* __restrict__ tile_off, uint8_t* __restrict__ code, uint32_t* __restrict__ bad)
{
  __shared__ uint32_t s_w[8];
  __shared__ uint8_t s_out[PASS ? FA_TILE : 16];
  __shared__ uint32_t s_raw[256 * FA_LSTRIDE];
  const uint64_t tile_base = (uint64_t)blockIdx.x * FA_TILE;
  const uint64_t base = tile_base + (uint64_t)threadIdx.x * 64;
  (void)bad;
  // (uniform) a whole tile of sequence lines -- no header line reaches into it: all but a few dozen of a genome's 180 000 tiles
  bool plain = false;
  int64_t r_tile = -1;
  if (tile_base + FA_TILE <= n) {
    r_tile = fa_header_before(hs, n_hdr, tile_base);
    plain = r_tile >= 0 && he[r_tile] < tile_base && ((uint64_t)(r_tile + 1) >= n_hdr || hs[r_tile + 1] >= tile_base + FA_TILE);
  }
  uint32_t cnt = 0;
  if (plain) {
    // the lane's 64 bytes in sixteen registers; a word without a byte below 0x21 is four bases, the others are looked at byte
    // by byte (line ends; white space by the rule of fa_is_base, through memory: it may look past the lane's bytes)
    uint32_t dw[16];
    fa_stage_tile(raw, tile_base, s_raw, dw);
    uint32_t keep16[16]; // per word: bit b = byte b is a base
#pragma unroll
    for (uint32_t w = 0; w < 16; ++w) {
      const uint32_t ctl = fa_bytes_ctl(dw[w]);
      uint32_t k4 = 0xFu;
      if (ctl) {
#pragma unroll
        for (uint32_t b = 0; b < 4; ++b)
          if ((ctl >> (8u * b + 7u)) & 1u) {
            const uint8_t c = (uint8_t)(dw[w] >> (8u * b));
            bool is = true;
            if (c == '\n' || c == '\r') {
              is = false;
            } else if (fa_is_blank(c)) {
              int64_t r = r_tile;
              is = fa_is_base(raw, n, base + 4u * w + b, hs, he, r, n_hdr);
            }
            if (!is) k4 &= ~(1u << b);
          }
      }
      keep16[w] = k4;
      cnt += (uint32_t)__popc(k4);
    }
    uint32_t total = 0;
    const uint32_t before = block_excl_scan_256(cnt, s_w, &total);
    if (PASS == 0) {
      if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
      return;
    }
    uint32_t o = before;
#pragma unroll
    for (uint32_t w = 0; w < 16; ++w) {
#pragma unroll
      for (uint32_t b = 0; b < 4; ++b)
        if ((keep16[w] >> b) & 1u) s_out[o++] = fa_code((uint8_t)(dw[w] >> (8u * b)));
    }
    __syncthreads();
    uint8_t* dst = code + tile_off[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < total; i += 256) dst[i] = s_out[i];
    return;
  }
  uint64_t keep = 0; // bit b: byte base + b is a base
  if (base < n) {
    const uint64_t end = min(base + 64, n);
    int64_t r = fa_header_before(hs, n_hdr, base);
    for (uint64_t i = base; i < end; ++i)
      if (fa_is_base(raw, n, i, hs, he, r, n_hdr)) {
        keep |= 1ull << (i - base);
        ++cnt;
      }
  }
  uint32_t total = 0;
  const uint32_t before = block_excl_scan_256(cnt, s_w, &total);
  if (PASS == 0) {
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
    return;
  }
  uint32_t o = before;
  while (keep) {
    const uint32_t b = (uint32_t)__ffsll((long long)keep) - 1u;
    keep &= keep - 1;
    s_out[o++] = fa_code(raw[base + b]);
  }
  __syncthreads();
  uint8_t* dst = code + tile_off[blockIdx.x];
  for (uint32_t i = threadIdx.x; i < total; i += 256) dst[i] = s_out[i];
}

// bases before byte pos[r] of the file (one workgroup per position).  With pos = the header starts: where record r starts in the
// genome; with pos = the ends of the first sequence lines: what the faidx column "bases per line" is the difference of.
__global__ __launch_bounds__(256) void k_fa_rec_off(const uint8_t* __restrict__ raw, uint64_t n, const uint64_t* __restrict__ hs,
                                                    const uint64_t* __restrict__ he, uint64_t n_hdr, const uint64_t* __restrict__ tile_off,
                                                    const uint64_t* __restrict__ pos, uint64_t* __restrict__ rec_off)
{
  __shared__ uint32_t s_cnt;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  const uint64_t r = blockIdx.x;
  const uint64_t at = min(pos[r], n);
  const uint64_t t = at / FA_TILE;
  uint32_t cnt = 0;
  for (uint64_t i = t * FA_TILE + threadIdx.x; i < at; i += 256) {
    int64_t q = fa_header_before(hs, n_hdr, i);
    cnt += fa_is_base(raw, n, i, hs, he, q, n_hdr) ? 1 : 0;
  }
  if (cnt) atomicAdd(&s_cnt, cnt);
  __syncthreads();
  if (threadIdx.x == 0) rec_off[r] = tile_off[t] + s_cnt;
}

// k-mer text of every minimizer (for `indexlr --seq` output when the host never held the bases)
__global__ __launch_bounds__(256) void k_mx_kmers(const uint8_t* __restrict__ code, const uint64_t* __restrict__ rec_off_dev,
                                                  const uint32_t* __restrict__ rec, const uint64_t* __restrict__ pos, uint64_t n, uint32_t k,
                                                  uint8_t* __restrict__ out)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t* s = code + rec_off_dev[rec[i]] + pos[i];
  uint8_t* o = out + i * k;
  for (uint32_t q = 0; q < k; ++q) {
    const uint8_t c = s[q];
    o[q] = c == 0 ? 'A' : c == 1 ? 'C' : c == 2 ? 'G' : c == 3 ? 'T' : 'N';
  }
}

// host -> device copy of a large pageable buffer through pinned staging on a few threads (the page-cache / mapping read is
// what limits one thread)
int fa_upload_raw(nts_ctx* ctx, const uint8_t* src, uint64_t n, uint8_t* d_dst, int fd = -1)
{
  // fd >= 0: the bytes are read from the file (page cache) straight into the pinned staging buffers with pread
  if (n == 0) return NTS_OK;
  if (n < ((uint64_t)64 << 20)) { // small file: one copy from the mapping, no threads (their fixed cost would be most of it)
    HIP_TRY(ctx, hipMemcpyAsync(d_dst, src, n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NTS_OK;
  }
  const uint64_t CHUNK = IO_CHUNK;
  const uint64_t n_chunks = (n + CHUNK - 1) / CHUNK;
  // (NTS_IO_THREADS: measurements; eight reader threads are the default)
  const unsigned want_threads = ctx->io_threads;
  const unsigned T = io_lanes(ctx, ctx->io_up, (unsigned)std::min<uint64_t>(n_chunks, want_threads));
  if (T == 0) return fail(ctx, NTS_ENOMEM, "FASTA upload: no pinned staging");
  std::atomic<uint64_t> next(0);
  std::atomic<bool> failed(false);
  const int device = ctx->device;
  auto worker = [&](unsigned lane) {
    if (hipSetDevice(device) != hipSuccess) {
      failed.store(true);
      return;
    }
    nts_ctx::IoLane& io = ctx->io_up[lane];
    hipStream_t st = io.stream;
    hipEvent_t done[2];
    hipEventCreateWithFlags(&done[0], hipEventDisableTiming);
    hipEventCreateWithFlags(&done[1], hipEventDisableTiming);
    bool used[2] = { false, false };
    int slot = 0;
    for (;;) {
      const uint64_t c = next.fetch_add(1);
      if (c >= n_chunks || failed.load()) break;
      const uint64_t len = std::min(CHUNK, n - c * CHUNK);
      if (used[slot] && hipEventSynchronize(done[slot]) != hipSuccess) failed.store(true);
      if (fd >= 0) {
        uint64_t got = 0;
        while (got < len) {
          const ssize_t r = pread(fd, io.stage[slot] + got, len - got, (off_t)(c * CHUNK + got));
          if (r <= 0) {
            failed.store(true);
            break;
          }
          got += (uint64_t)r;
        }
      } else {
        memcpy(io.stage[slot], src + c * CHUNK, len);
      }
      if (hipMemcpyAsync(d_dst + c * CHUNK, io.stage[slot], len, hipMemcpyHostToDevice, st) != hipSuccess) failed.store(true);
      hipEventRecord(done[slot], st);
      used[slot] = true;
      slot ^= 1;
    }
    hipStreamSynchronize(st);
    hipEventDestroy(done[0]);
    hipEventDestroy(done[1]);
  };
  std::vector<std::thread> pool;
  for (unsigned t = 0; t < T; ++t) pool.emplace_back(worker, t);
  for (auto& th : pool) th.join();
  return failed.load() ? fail(ctx, NTS_EHIP, "FASTA upload failed") : NTS_OK;
}

} // namespace

extern "C" int nts_genome_from_fasta(nts_ctx* ctx, const char* path, nts_genome** out, nts_fasta* meta)
{
  if (!ctx || !path || !out || !meta) return fail(ctx, NTS_EINVAL, "nts_genome_from_fasta: bad arguments");
  memset(meta, 0, sizeof(*meta));
  *out = nullptr;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const bool trace = NTS_KNOB("NTS_FASTA_DEBUG") != nullptr; // lap times on stderr
  auto t_last = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (!trace) return;
    hipStreamSynchronize(ctx->stream);
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "nts_genome_from_fasta %-12s %.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
    t_last = now;
  };
  const uint8_t* raw = nullptr;
  uint64_t n = 0;
  void* fh = nullptr;
  if (nts_internal_file_open(path, &raw, &n, &fh) != NTS_OK) return fail(ctx, NTS_EINVAL, std::string("cannot read ") + path);
  lap("open");
  struct Closer
  {
    void* h;
    ~Closer() { nts_internal_file_close(h); }
  } closer{ fh };
  {
    uint64_t q = 0;
    while (q < n && (raw[q] == '\n' || raw[q] == '\r' || raw[q] == ' ' || raw[q] == '\t')) ++q;
    if (q < n && raw[q] == '@') return fail(ctx, NTS_EFORMAT, std::string(path) + " is not FASTA (FASTQ?)");
    if (q == n) n = 0; // blank file: no records
  }
  const uint64_t n_tiles = (n + FA_TILE - 1) / FA_TILE;
  uint64_t n_hdr = 0, n_seq = 0;
  std::vector<uint64_t> hs, he, le, roff, lcnt; // lcnt[r]: bases before the end of record r's first sequence line
  uint8_t* d_raw = nullptr;
  uint64_t *d_hs = nullptr, *d_he = nullptr, *d_toff = nullptr;
  if (n) {
    d_raw = (uint8_t*)ws_get(ctx, "fa_raw", n + 64);
    if (!d_raw) return NTS_ENOMEM;
    int fd = -1;
    {
      const std::string sp(path);
      if (!(sp.size() >= 3 && sp.compare(sp.size() - 3, 3, ".gz") == 0)) fd = open(path, O_RDONLY);
      struct stat st;
      if (fd >= 0 && (fstat(fd, &st) != 0 || (uint64_t)st.st_size != n)) {
        close(fd);
        fd = -1;
      }
    }
    lap("workspace");
    const int rc_up = fa_upload_raw(ctx, raw, n, d_raw, fd);
    if (fd >= 0) close(fd);
    if (rc_up) return rc_up;
    lap("upload");
    NTS_WS(d_tnl, uint64_t*, "fa_tile_nl", n_tiles * 8);
    NTS_WS(d_ctl, unsigned long long*, "fa_ctl", 64);
    uint64_t cap = std::max<uint64_t>(1024, n / 4096);
    for (int attempt = 0;; ++attempt) {
      NTS_WS(d_hdr, uint64_t*, "fa_hdr", cap * 8);
      HIP_TRY(ctx, hipMemsetAsync(d_ctl, 0, 64, ctx->stream));
      NTS_LAUNCH(k_fa_scan, dim3((uint32_t)n_tiles), dim3(256), 0, ctx->stream, d_raw, n, d_hdr, cap, d_ctl, d_tnl);
      unsigned long long cnt = 0;
      HIP_TRY(ctx, hipMemcpyAsync(&cnt, d_ctl, 8, hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      n_hdr = cnt;
      if (n_hdr <= cap) break;
      if (attempt) return fail(ctx, NTS_EHIP, "nts_genome_from_fasta: header count changed");
      cap = n_hdr;
    }
    lap("scan");
    if (n_hdr == 0) return fail(ctx, NTS_EFORMAT, std::string(path) + " is not FASTA (no '>' header)");
    if (n_hdr >= 0xFFFFFFF0ULL) return fail(ctx, NTS_ERANGE, "nts_genome_from_fasta: too many records");
    uint64_t* d_hdr = (uint64_t*)ws_get(ctx, "fa_hdr", cap * 8);
    d_hs = (uint64_t*)ws_get(ctx, "fa_hs", n_hdr * 8);
    d_he = (uint64_t*)ws_get(ctx, "fa_he", n_hdr * 8);
    NTS_WS(d_le, uint64_t*, "fa_le", n_hdr * 8);
    NTS_WS(d_roff, uint64_t*, "fa_roff", n_hdr * 8);
    if (!d_hs || !d_he) return NTS_ENOMEM;
    size_t tmp = 0;
    HIP_TRY(ctx, rocprim::radix_sort_keys(nullptr, tmp, d_hdr, d_hs, n_hdr, 0, 64, ctx->stream));
    NTS_WS(d_tmp, void*, "fa_sort_tmp", tmp);
    HIP_TRY(ctx, rocprim::radix_sort_keys(d_tmp, tmp, d_hdr, d_hs, n_hdr, 0, 64, ctx->stream));
    NTS_LAUNCH(k_fa_headers, dim3((uint32_t)n_hdr), dim3(256), 0, ctx->stream, d_raw, n, d_hs, n_hdr, d_tnl, n_tiles, d_he, d_le);
    // bases per tile -> offsets
    NTS_WS(d_tcnt, uint64_t*, "fa_tile_cnt", (n_tiles + 1) * 8);
    d_toff = (uint64_t*)ws_get(ctx, "fa_tile_off", (n_tiles + 1) * 8);
    if (!d_toff) return NTS_ENOMEM;
    HIP_TRY(ctx, hipMemsetAsync(d_tcnt + n_tiles, 0, 8, ctx->stream));
    NTS_LAUNCH(k_fa_bases<0>, dim3((uint32_t)n_tiles), dim3(256), 0, ctx->stream, d_raw, n, d_hs, d_he, n_hdr, d_tcnt, (const uint64_t*)nullptr,
                       (uint8_t*)nullptr, (uint32_t*)(d_ctl + 1));
    size_t tmp2 = 0;
    HIP_TRY(ctx, rocprim::exclusive_scan(nullptr, tmp2, d_tcnt, d_toff, (uint64_t)0, n_tiles + 1, rocprim::plus<uint64_t>(), ctx->stream));
    NTS_WS(d_tmp2, void*, "fa_scan_tmp", tmp2);
    HIP_TRY(ctx, rocprim::exclusive_scan(d_tmp2, tmp2, d_tcnt, d_toff, (uint64_t)0, n_tiles + 1, rocprim::plus<uint64_t>(), ctx->stream));
    NTS_LAUNCH(k_fa_rec_off, dim3((uint32_t)n_hdr), dim3(256), 0, ctx->stream, d_raw, n, d_hs, d_he, n_hdr, d_toff, d_hs, d_roff);
    NTS_WS(d_lcnt, uint64_t*, "fa_lcnt", n_hdr * 8);
    NTS_LAUNCH(k_fa_rec_off, dim3((uint32_t)n_hdr), dim3(256), 0, ctx->stream, d_raw, n, d_hs, d_he, n_hdr, d_toff, d_le, d_lcnt);
    hs.resize(n_hdr);
    he.resize(n_hdr);
    le.resize(n_hdr);
    roff.resize(n_hdr);
    lcnt.resize(n_hdr);
    HIP_TRY(ctx, hipMemcpyAsync(lcnt.data(), d_lcnt, n_hdr * 8, hipMemcpyDeviceToHost, ctx->stream));
    unsigned long long ctl[2] = { 0, 0 };
    HIP_TRY(ctx, hipMemcpyAsync(&n_seq, d_toff + n_tiles, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctl, d_ctl, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(hs.data(), d_hs, n_hdr * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(he.data(), d_he, n_hdr * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(le.data(), d_le, n_hdr * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(roff.data(), d_roff, n_hdr * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  lap("tables");
  // ---- the genome
  nts_genome* g = new nts_genome();
  g->n = n_seq;
  g->n_rec = (uint32_t)n_hdr;
  g->rec_off = roff;
  g->rec_len.resize(n_hdr);
  for (uint64_t r = 0; r < n_hdr; ++r) g->rec_len[r] = (r + 1 < n_hdr ? roff[r + 1] : n_seq) - roff[r];
  g->total_bases = n_seq;
  if (dev_malloc((void**)&g->d_code, PAD + n_seq + PAD) != hipSuccess) {
    delete g;
    return fail(ctx, NTS_ENOMEM, "hipMalloc genome");
  }
  hipMemsetAsync(g->d_code, CODE_INVALID, PAD, ctx->stream);
  hipMemsetAsync(g->d_code + PAD + n_seq, CODE_INVALID, PAD, ctx->stream);
  if (n)
    NTS_LAUNCH(k_fa_bases<1>, dim3((uint32_t)n_tiles), dim3(256), 0, ctx->stream, d_raw, n, d_hs, d_he, n_hdr, (uint64_t*)nullptr, d_toff,
                       g->d_code + PAD, (uint32_t*)ws_get(ctx, "fa_ctl", 64) + 4);
  lap("encode");
  if (int rc = nts_genome_finish_impl(ctx, g)) {
    dev_free(g->d_code);
    dev_free(g->d_rec_off);
    delete g;
    return rc;
  }
  lap("finish");
  // ---- record ids and faidx columns from the header lines (the only bytes the host looks at)
  std::string names;
  std::vector<uint64_t> fai_off(n_hdr);
  std::vector<uint32_t> fai_bases(n_hdr, 0), fai_width(n_hdr, 0);
  for (uint64_t r = 0; r < n_hdr; ++r) {
    uint64_t s = hs[r] + 1, e = s;
    while (e < he[r] && raw[e] != ' ' && raw[e] != '\t' && raw[e] != '\r' && raw[e] != '\v' && raw[e] != '\f') ++e;
    names.append((const char*)raw + s, e - s);
    names.push_back('\0');
    fai_off[r] = he[r] < n ? he[r] + 1 : n;
    const uint64_t ls = he[r] + 1;
    if (ls < n && raw[ls] != '>' && le[r] > ls && g->rec_len[r]) {
      const uint64_t len = le[r] - ls;
      // bases of the first line: counted on the device (the host must not walk the mapping: in single-line FASTA that line is
      // the whole chromosome) -- what lies between the record's start and the end of that line
      const uint64_t bases = lcnt[r] - roff[r];
      fai_bases[r] = (uint32_t)bases;
      fai_width[r] = (uint32_t)(len + (le[r] < n ? 1 : 0));
    }
  }
  auto dup = [](const void* src, size_t bytes) {
    void* p = malloc(std::max<size_t>(bytes, 1));
    if (p && bytes) memcpy(p, src, bytes);
    return p;
  };
  meta->seq = nullptr;
  meta->n = n_seq;
  meta->n_rec = (uint32_t)n_hdr;
  meta->rec_off = (uint64_t*)dup(g->rec_off.data(), n_hdr * 8);
  meta->rec_len = (uint64_t*)dup(g->rec_len.data(), n_hdr * 8);
  meta->names_bytes = names.size();
  meta->names = (char*)dup(names.data(), names.size());
  meta->fai_offset = (uint64_t*)dup(fai_off.data(), n_hdr * 8);
  meta->fai_linebases = (uint32_t*)dup(fai_bases.data(), n_hdr * 4);
  meta->fai_linewidth = (uint32_t*)dup(fai_width.data(), n_hdr * 4);
  if (!meta->rec_off || !meta->rec_len || !meta->names || !meta->fai_offset || !meta->fai_linebases || !meta->fai_linewidth) {
    nts_fasta_free(meta);
    nts_genome_free(ctx, g);
    return fail(ctx, NTS_ENOMEM, "nts_genome_from_fasta: host allocation failed");
  }
  lap("names");
  *out = g;
  return NTS_OK;
}

extern "C" int nts_ingest_trim(nts_ctx* ctx)
{
  if (!ctx) return NTS_EINVAL;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (auto it = ctx->ws.begin(); it != ctx->ws.end();) {
    if (it->first.compare(0, 3, "fa_") == 0) {
      if (it->second.first) dev_free(it->second.first);
      it = ctx->ws.erase(it);
    } else
      ++it;
  }
  io_release(ctx->io_up);
  return NTS_OK;
}

// The Bloom build's buckets (13 + 11 GB at 3 Gbp: two thirds of what a run holds while its filter is made) are dead once the common filter
// stands -- rule indexlr and stage 3 build nothing (bin/ntsynt_run_pipeline.smk:74-103).  Given back here they stay in the library's
// allocation cache, and what follows (the sketch's 4 GB of workspaces, the graph stage) is cut from them instead of asked of the driver.
extern "C" int nts_bf_build_trim(nts_ctx* ctx)
{
  if (!ctx) return NTS_EINVAL;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (auto it = ctx->ws.begin(); it != ctx->ws.end();) {
    if (it->first.compare(0, 4, "bin_") == 0) {
      if (it->second.first) dev_free(it->second.first);
      it = ctx->ws.erase(it);
    } else
      ++it;
  }
  return NTS_OK;
}

// k-mer text (upper case, k bytes each, no separators) of every minimizer of `mx`, sketched from `g`: what `indexlr --seq`
// prints (bin/ntsynt_run_pipeline.smk:81), for callers that never held the bases on the host
extern "C" int nts_mx_kmers(nts_ctx* ctx, const nts_genome* g, const nts_mx* mx, uint32_t k, uint8_t* host)
{
  if (!ctx || !g || !mx || k == 0 || (mx->n && !host)) return fail(ctx, NTS_EINVAL, "nts_mx_kmers: bad arguments");
  if (mx->n == 0) return NTS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  uint8_t* d = (uint8_t*)ws_get(ctx, "mx_kmers", mx->n * k);
  if (!d) return NTS_ENOMEM;
  NTS_LAUNCH(k_mx_kmers, dim3((uint32_t)((mx->n + 255) / 256)), dim3(256), 0, ctx->stream, g->d_code + PAD, g->d_rec_off, mx->d_rec, mx->d_pos,
                     mx->n, k, d);
  HIP_TRY(ctx, hipMemcpyAsync(host, d, mx->n * k, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return NTS_OK;
}

// ---- one workgroup hashes one tile of consecutive k-mers: the sweep every interval kernel is built on ---------------------------------
// A tile is up to KEY_TILE = 256 lanes x 32 consecutive valid k-mers whose bases are contiguous in the genome's code array
// (nts_iv_cut.inc cuts intervals into such tiles on the host; k_hash's fast path finds them in its run table).  The workgroup
//   1. loads the roll and seed tables into s_tab[36]                                                     (tab_load),
//   2. k <= FAST_K_MAX: stages the tile's bases into s_seq with 16-byte loads, 4 bytes of padding per 32 -- a lane's 32 + k - 1
//      bases start 36 bytes after its neighbour's, so the lanes' byte reads are conflict-free            (seq_stage, BaseLds);
//      k > FAST_K_MAX: the bases do not fit the staging area, every lane reads its own from the L2       (BaseMem),
//   3. has every lane hash its first k-mer from the init table and roll on, eight k-mers at a time; every hash and every batch of
//      eight go to the kernel's own policy -- probe, sample, insert                                         (lane_sweep),
//   4. where the tile's result is one number, adds the lanes up and stores it with one plain store       (block_sum_store).
// tile_enter is 1 + 2 + the barrier for a tile given by position and length; TileLane::sweep is 3 on whichever accessor applies.
// SEQ_LDS_DWORDS, FAST_K_MAX and the 36-byte lane stride belong to this layout: seq_stage and BaseLds are its definition.
//   bytes read: staging reads whole 16-byte words around the tile's bases, at most 15 bytes before and after.  A lane with fewer than
//   32 k-mers finishes its batch of eight, so it rolls on for at most seven positions and fetches up to eight bases beyond the tile's
//   last one -- from stale staging bytes below FAST_K_MAX (inside s_seq: 15 + 8192 + 127 bytes is what SEQ_LDS_DWORDS holds), from
//   memory above it.  Both kinds of excess stay inside the genome's code array, which carries PAD = 256 invalid bytes before its
//   first and after its last base, also where a tile ends on the genome's last base; accessors mask to two bits and what is hashed
//   there is never used (policies test `j < n_mine`).

__device__ __forceinline__ void tab_load(uint64_t* s_tab, const HashParams& hp, uint32_t tid)
{
  if (tid < 16) {
    s_tab[tid] = hp.roll_f[tid];
    s_tab[16 + tid] = hp.roll_r[tid];
  }
  if (tid < 4) s_tab[32 + tid] = hp.seed[tid];
}

// the bases of the tile_len k-mers from code[pos] on into the padded layout; returns a = pos % 16, the offset of base 0 in it
__device__ __forceinline__ uint32_t seq_stage(uint32_t* s_seq, const uint8_t* __restrict__ code, uint64_t pos, uint32_t tile_len, uint32_t k,
                                              uint32_t tid)
{
  const uint32_t a = (uint32_t)(pos & 15u);
  const uint8_t* src = code + (pos - a);
  const uint32_t n_bytes = a + tile_len + k - 1;
  const uint32_t n16 = (n_bytes + 15u) >> 4;
  for (uint32_t c = tid; c < n16; c += HASH_THREADS) {
    const uint4 v = *reinterpret_cast<const uint4*>(src + 16u * c);
    const uint32_t d = 4u * c + (c >> 1);
    s_seq[d] = v.x;
    s_seq[d + 1] = v.y;
    s_seq[d + 2] = v.z;
    s_seq[d + 3] = v.w;
  }
  return a;
}

struct BaseLds // base i of a lane's stretch, staged: s0 = a + the lane's first k-mer
{
  const uint8_t* sb;
  uint32_t s0;
  __device__ __forceinline__ uint32_t operator()(uint32_t i) const
  {
    const uint32_t s = s0 + i;
    return sb[s + 4u * (s >> 5)] & 3u;
  }
};

struct BaseMem // the same from memory: p = the lane's first base (a tile lies inside one stretch of valid bases: plain offsets)
{
  const uint8_t* p;
  __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return p[i] & 3u; }
};

// from the k-mer at base s of the stretch to the one at s + 1
template <typename BaseAt>
__device__ __forceinline__ void hash_roll(const uint64_t* s_tab, BaseAt&& base, uint32_t s, uint32_t k, uint64_t& f, uint64_t& r)
{
  const uint32_t cout = base(s), cin = base(s + k);
  f = srol1(f) ^ s_tab[cin * 4 + cout];
  r = sror1(r ^ s_tab[16 + cin * 4 + cout]);
}

// a lane's n_mine (1 .. 32) k-mers, eight at a time: each(j, u, h) receives the hash of k-mer j = b0 + u as soon as it is rolled -- a
// policy issues its loads there --, after(b0) follows the batch's eighth (k-mers at and beyond n_mine are not the tile's: see "bytes
// read" above).  What a policy keeps between the two is an array of eight indexed by u: registers, once the batch is unrolled.
template <typename BaseAt, typename Each, typename After>
__device__ __forceinline__ void lane_sweep(const HashParams& hp, const uint64_t* s_tab, uint32_t n_mine, BaseAt&& base, Each&& each, After&& after)
{
  uint64_t f = 0, r = 0;
  hash_init(hp, base, f, r);
  uint32_t s = 0;
#pragma unroll 1
  for (uint32_t b0 = 0; b0 < 32; b0 += 8) {
    if (b0 >= n_mine) break;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      each(b0 + u, u, f + r);
      hash_roll(s_tab, base, s++, hp.k, f, r);
    }
    after(b0);
  }
}

struct TileLane // what a lane of the tile's workgroup hashes: k-mers first .. first + n_mine - 1 of the tile (n_mine = 0: none)
{
  uint32_t first, n_mine;
  bool staged;
  BaseLds lds;
  BaseMem mem;
  template <typename Each, typename After>
  __device__ __forceinline__ void sweep(const HashParams& hp, const uint64_t* s_tab, Each&& each, After&& after) const
  {
    if (!n_mine) return;
    if (staged)
      lane_sweep(hp, s_tab, n_mine, lds, each, after);
    else
      lane_sweep(hp, s_tab, n_mine, mem, each, after);
  }
};

// tables, staging, barrier: every lane of the workgroup calls it, with the tile's first k-mer at code[pos] and len (<= KEY_TILE) k-mers
__device__ __forceinline__ TileLane tile_enter(uint64_t* s_tab, uint32_t* s_seq, const uint8_t* __restrict__ code, uint64_t pos, uint32_t len,
                                               const HashParams& hp)
{
  const uint32_t tid = threadIdx.x;
  tab_load(s_tab, hp, tid);
  const uint32_t tile_len = min(len, KEY_TILE);
  TileLane t;
  t.first = 32u * tid;
  t.n_mine = t.first < tile_len ? min(32u, tile_len - t.first) : 0u;
  t.staged = hp.k <= FAST_K_MAX;
  uint32_t a = 0;
  if (t.staged) a = seq_stage(s_seq, code, pos, tile_len, hp.k, tid);
  __syncthreads();
  t.lds = BaseLds{ reinterpret_cast<const uint8_t*>(s_seq), a + t.first };
  t.mem = BaseMem{ code + pos + t.first };
  return t;
}

// the workgroup's sum of v into *dst: lanes -> wave -> workgroup (s_w[HASH_THREADS / 64]), one plain store by one lane
__device__ __forceinline__ void block_sum_store(uint32_t v, uint32_t* s_w, uint32_t* __restrict__ dst)
{
  const uint32_t tid = threadIdx.x;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  if ((tid & 63u) == 0) s_w[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) {
    uint32_t sum = 0;
#pragma unroll
    for (int wv = 0; wv < HASH_THREADS / 64; ++wv) sum += s_w[wv];
    *dst = sum;
  }
}

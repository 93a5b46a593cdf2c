// Pruned sketch path (included inside the anonymous namespace of ntsynt_hip.hip).
//
// Exactness argument.  Keys: x_j = h0_j if the common filter accepts k-mer j, else ~0.  Fix a threshold
// tau < ~0 and let S = { j : h0_j <= tau and the filter accepts j } ("candidates").  Every k-mer outside
// S has x_j > tau.  So for a window W (w consecutive valid k-mers) with W ∩ S != {} the rightmost argmin
// of x over W lies in S and is decided by S ∩ W alone; only k-mers with h0 <= tau are ever probed.
// Windows with W ∩ S == {} ("uncovered") lie strictly between two consecutive candidates (or a record
// end) that are >= w apart; those index ranges are handed to the dense kernels unchanged.  The union of
// both emissions is the dense result; no window is evaluated twice.
//
//   k_hash_select : all k-mers -> ordered candidate lists per key tile (hash once, probe ~c/w of them)
//   k_cand_compact: tile lists -> one ordered array (PJ, PK)
//   k_sparse_win  : per candidate, nearest smaller to the left / smaller-or-equal to the right within w
//                   => is it the rightmost minimum of some window?  + uncovered ranges between candidates
//                   (and whole records without any candidate)
constexpr uint32_t SEL_CAP = 2048;       // candidates staged in LDS per round
constexpr uint32_t SEL_PER_LANE = 64;    // consecutive k-mers rolled by one lane (init cost k/64)
// fast path: private candidate slots per lane = template parameter of k_hash_select (8, or 16 when c/w is large)
constexpr uint32_t SEL_TILE = HASH_THREADS * SEL_PER_LANE; // 16384 compact indices per workgroup
constexpr uint32_t SPARSE_THREADS = 256;
constexpr uint32_t SPARSE_ITEMS = 2;    // candidates per lane of k_sparse_win: one staging pass (one round trip to memory) serves that many rounds
constexpr uint32_t SPARSE_BLOCK = SPARSE_THREADS * SPARSE_ITEMS;
constexpr uint32_t CC_TILES = 8;         // tiles per workgroup of k_cand_compact

struct SelParams
{
  const uint8_t* code;
  const uint32_t* pack; // the bases 2 bits each, 16 per word (nts_genome::d_pack)
  const uint64_t* run_pos;
  const uint64_t* run_vstart;
  uint32_t n_runs;
  uint64_t n_valid;
  HashParams hp;
  const uint32_t* bf; // nullptr: no filter, every candidate passes
  FastMod fm;
  uint64_t tau;
  uint32_t flush_at; // fast path: probe the parked candidates before a block of 16 steps once more than this many slots are
                     // in use (slots minus what a block may add; = slots when one batch at the end is enough)
  uint64_t* seg_j; // N_SEG segments of seg_cap candidates each
  uint64_t* seg_key;
  uint64_t seg_cap;
  unsigned long long* seg_count;
  uint64_t* tile_off; // directory: offset of the tile's list inside its segment
  uint32_t* tile_cnt; //            and its length
  uint8_t* tile_ordered; //         1 = the list is already in index order (fast path), 0 = k_cand_compact sorts it
  uint32_t w_elim;       // k_hash_select_hi: window length when it may drop candidates that cannot be a window's minimum (0: keep all)
};




// Hash every k-mer of a 16384-index tile, keep the k-mers with h0 <= tau ("candidates"), probe them and write the
// accepted ones to the tile's slice of a segment; order across tiles is kept by the directory.
//   Fast path (tile inside one run, at most SEL_SLOTS ACCEPTED candidates per lane): a lane parks its candidates in
//   its own LDS slots, probes them in batches whenever the slots are full and keeps the accepted ones -- no atomics,
//   and the tile's list comes out in index order, so k_cand_compact only copies it.  The
//   lane's outgoing and incoming bases sit in eight registers (2 bits each, from the packed image of the genome),
//   the 64 rolling steps are unrolled: per step one shift-mask-or for the roll-table offset, two LDS table reads.
//   General path (tile crosses runs, or some lane has more candidates): candidates are appended to one list with
//   an LDS atomic each (unordered; k_cand_compact sorts), and a tile with more than SEL_CAP candidates (tau covering
//   > 12 % of the hash range, or repeats) is processed in 8 passes over index ranges of 2048.
template <uint32_t SEL_SLOTS>
__global__ __launch_bounds__(HASH_THREADS) void k_hash_select(SelParams P)
{
  // one block of LDS with the roll tables at offset 0: their address is then the table offset itself (the rolling
  // loop forms it once per step)
  struct Lds
  {
    uint64_t tab[36];
    uint64_t ch[(SEL_SLOTS + 1) * HASH_THREADS]; // >= SEL_CAP entries: [slot][lane] (+ a spare row) on the fast path, one list on the general path
    uint16_t ci[SEL_SLOTS * HASH_THREADS];
    uint32_t ctl[4]; // [0] appended this pass, [1] accepted so far / write cursor
    unsigned long long base;
  };
  __shared__ Lds lds;
  uint64_t* const s_tab = lds.tab;
  uint64_t* const s_ch = lds.ch;
  uint16_t* const s_ci = lds.ci;
  uint32_t* const s_ctl = lds.ctl;
  unsigned long long& s_base = lds.base;
  const uint32_t tid = threadIdx.x;
  if (tid < 16) {
    s_tab[tid] = P.hp.roll_f[tid];
    s_tab[16 + tid] = P.hp.roll_r[tid];
  }
  if (tid < 4) s_tab[32 + tid] = P.hp.seed[tid];
  if (tid == 0) s_ctl[0] = s_ctl[1] = 0;
  const uint32_t k = P.hp.k;
  const uint64_t tile = blockIdx.x;
  const uint64_t J0 = tile * SEL_TILE;
  const uint32_t tile_len = (uint32_t)min((uint64_t)SEL_TILE, P.n_valid - J0);
  uint32_t lo = 0, hi = P.n_runs;
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (P.run_vstart[mid] <= J0)
      lo = mid;
    else
      hi = mid;
  }
  const uint64_t v0 = P.run_vstart[lo], v1 = P.run_vstart[lo + 1];
  const bool single = (J0 + tile_len <= v1) && (k <= FAST_K_MAX);
  // the unrolled loop compares high words only: exact when the low word of tau is all ones (what the host passes,
  // except for the "every k-mer is a candidate" setting, which then simply takes the general path)
  const bool hi_only = (uint32_t)P.tau == 0xFFFFFFFFu;
  const uint32_t first = SEL_PER_LANE * tid;
  const uint32_t n_mine = first < tile_len ? min(SEL_PER_LANE, tile_len - first) : 0u;
  const uint64_t tau = P.tau;
  // tile inside one run: all of its bases are valid and come from the 2-bit image of the genome
  const uint64_t P0 = single ? P.run_pos[lo] + (J0 - v0) : 0; // genome position of the tile's first base
  auto base_abs = [&](uint64_t p) -> uint32_t { return (P.pack[p >> 4] >> (2u * ((uint32_t)p & 15u))) & 3u; };
  __syncthreads();

  // one pass over the lane's k-mers: append candidates whose tile index lies in [r_lo, r_hi)
  auto roll_pass = [&](uint32_t r_lo, uint32_t r_hi) {
    if (n_mine == 0 || first >= r_hi || first + n_mine <= r_lo) return;
    auto consider = [&](uint64_t h, uint32_t idx) {
      if (h <= tau && idx >= r_lo && idx < r_hi) {
        const uint32_t slot = atomicAdd(&s_ctl[0], 1u);
        if (slot < SEL_CAP) {
          s_ch[slot] = h;
          s_ci[slot] = (uint16_t)idx;
        }
      }
    };
    if (single) {
      uint64_t s = P0 + first;
      uint64_t f = 0, r = 0;
      hash_init(P.hp, [&](uint32_t i) { return base_abs(s + i); }, f, r);
      for (uint32_t u = 0; u < n_mine; ++u) {
        consider(f + r, first + u);
        const uint32_t cout = base_abs(s), cin = base_abs(s + k);
        f = srol1(f) ^ s_tab[cin * 4 + cout];
        r = sror1(r ^ s_tab[16 + cin * 4 + cout]);
        ++s;
      }
    } else {
      uint64_t j = J0 + first;
      const uint64_t j_end = j + n_mine;
      uint32_t rl = 0, rh = P.n_runs;
      while (rh - rl > 1) {
        const uint32_t mid = rl + ((rh - rl) >> 1);
        if (P.run_vstart[mid] <= j)
          rl = mid;
        else
          rh = mid;
      }
      uint32_t ri = rl;
      while (j < j_end) {
        const uint64_t rv0 = P.run_vstart[ri], rv1 = P.run_vstart[ri + 1];
        const uint64_t seg_end = min(j_end, rv1);
        uint64_t p = P.run_pos[ri] + (j - rv0);
        uint64_t f = 0, r = 0;
        for (uint32_t i = 0; i < k; ++i) {
          f = srol1(f) ^ s_tab[32 + P.code[p + i]];
          r = srol1(r) ^ s_tab[32 + 3 - P.code[p + k - 1 - i]];
        }
        for (;;) {
          consider(f + r, (uint32_t)(j - J0));
          ++j;
          if (j >= seg_end) break;
          const uint32_t cout = P.code[p], cin = P.code[p + k];
          f = srol1(f) ^ s_tab[cin * 4 + cout];
          r = sror1(r ^ s_tab[16 + cin * 4 + cout]);
          ++p;
        }
        ++ri;
      }
    }
  };
  // probe the staged candidates; returns a bit mask of this lane's accepted entries (entry e = tid + 256*i)
  auto probe_staged = [&](uint32_t n, uint32_t* n_acc) -> uint32_t {
    uint32_t bits = 0, cnt = 0;
    for (uint32_t i = 0, e = tid; e < n; e += HASH_THREADS, ++i) {
      bool ok = true;
      if (P.bf != nullptr) ok = bf_test(P.bf, P.fm(s_ch[e]));
      if (ok) {
        bits |= 1u << i;
        ++cnt;
      }
    }
    *n_acc = cnt;
    return bits;
  };
  auto write_staged = [&](uint32_t n, uint32_t bits, uint64_t dst_base) {
    uint64_t* dj = P.seg_j + dst_base;
    uint64_t* dk = P.seg_key + dst_base;
    for (uint32_t i = 0, e = tid; e < n; e += HASH_THREADS, ++i) {
      if ((bits >> i) & 1u) {
        const uint32_t slot = atomicAdd(&s_ctl[1], 1u);
        dj[slot] = J0 + s_ci[e];
        dk[slot] = s_ch[e];
      }
    }
  };
  const uint32_t seg = (uint32_t)(tile % N_SEG);
  __shared__ uint32_t s_w[8];

  if (hi_only && k <= FAST_K_MAX) {
    // ---- fast path ---------------------------------------------------------------------------------------------
    // The lane's slots hold [accepted candidates ..., candidates not probed yet ...], in index order.  Before a block
    // of 16 steps that could fill them, the unprobed ones are probed together (independent loads) and the accepted
    // ones close ranks; the same happens once more after the last step.  With few candidates per lane (c/w small,
    // 8 slots) that is one batch at the end; with many (16 slots) a batch per block, and a lane keeps going as long as
    // the ACCEPTED candidates plus one block's worth fit.
    // Slots are addressed by a byte cursor (row = slot, column = lane); the step index of a candidate is not stored
    // but kept as a bit in a 64-bit mask per lane (slot i of the lane <-> i-th set bit), so that a hit costs one LDS
    // write and three integer operations.  Hits beyond the slots land in a spare row; the cursor keeps counting, which
    // is how the overflow is seen.
    constexpr uint32_t ROW = HASH_THREADS * 8u;
    static_assert(ROW == 2048u, "cursor >> 11 is the slot count");
    uint8_t* const ch_bytes = reinterpret_cast<uint8_t*>(s_ch);
    const uint32_t lane_ofs = tid * 8u;
    const uint32_t spare = SEL_SLOTS * ROW + lane_ofs;
    uint32_t cur = lane_ofs;            // byte cursor: slots in use = cur >> 11
    uint32_t acc = 0;                   // of which already probed and accepted
    uint32_t pen_lo = 0, pen_hi = 0;    // steps whose candidate is parked but not probed yet
    uint64_t acc_mask = 0;              // steps whose candidate was accepted
    bool over = false;                  // more accepted candidates than slots: the tile goes through the general path
    const uint32_t tau_hi = (uint32_t)(tau >> 32);
    uint64_t f = 0, r = 0;
    auto flush = [&]() {
      const uint32_t cnt = cur >> 11;
      if (cnt > SEL_SLOTS) {
        over = true;
        return;
      }
      uint64_t pen = ((uint64_t)pen_hi << 32) | pen_lo;
      pen_lo = pen_hi = 0;
      if (P.bf == nullptr) {
        acc_mask |= pen;
        acc = cnt;
        return;
      }
      uint32_t wd[SEL_SLOTS], bit[SEL_SLOTS];
#pragma unroll
      for (uint32_t i = 0; i < SEL_SLOTS; ++i) {
        wd[i] = 0;
        bit[i] = 0;
        if (acc + i < cnt) {
          const uint64_t idx = P.fm(s_ch[(acc + i) * HASH_THREADS + tid]);
          wd[i] = P.bf[idx >> 5];
          bit[i] = (uint32_t)idx & 31u;
        }
      }
      uint32_t wpos = acc;
#pragma unroll
      for (uint32_t i = 0; i < SEL_SLOTS; ++i) {
        if (acc + i < cnt) {
          const uint64_t lowest = pen & (0 - pen);
          pen ^= lowest;
          if ((wd[i] >> bit[i]) & 1u) {
            if (wpos != acc + i) s_ch[wpos * HASH_THREADS + tid] = s_ch[(acc + i) * HASH_THREADS + tid];
            acc_mask |= lowest;
            ++wpos;
          }
        }
      }
      acc = wpos;
      cur = wpos * ROW + lane_ofs;
    };
    // t8 = 8 * (4 * incoming base + outgoing base): byte offset into the roll tables; t = step number of the lane
    auto step = [&](uint32_t t8, uint32_t t) {
      // f + r as two 32-bit halves: the test below is then a 32-bit compare of the high half (written as
      // (uint32_t)(h >> 32) <= tau_hi the optimiser widens it to a 64-bit compare of a zero-extended copy)
      typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
      u32x2 hv;
      asm("v_lshl_add_u64 %0, %1, 0, %2" : "=v"(hv) : "v"(f), "v"(r));
      const uint64_t h = ((uint64_t)hv.y << 32) | hv.x;
      if (hv.y <= tau_hi) {        // == (h <= tau): the host passes tau with its low 32 bits set
        *reinterpret_cast<uint64_t*>(ch_bytes + min(cur, spare)) = h;
        cur += ROW;
        if (t < 32u)
          pen_lo |= 1u << t;
        else
          pen_hi |= 1u << (t - 32u);
      }
      const uint64_t tf = *reinterpret_cast<const uint64_t*>(reinterpret_cast<const uint8_t*>(s_tab) + t8);
      const uint64_t tr = *reinterpret_cast<const uint64_t*>(reinterpret_cast<const uint8_t*>(s_tab) + 128 + t8);
      f = srol1(f) ^ tf;
      r = sror1(r ^ tr);
    };
    // the run holding the lane's first k-mer (a tile of a fragmented assembly spans several runs: contig ends, N
    // stretches; each lane looks its own run up)
    const uint64_t j_lane = J0 + first;
    uint32_t run = lo;
    bool shared_lane = false; // the lane's k-mers end with the tile or cross into another run: hashed by the whole wave below
    if (n_mine) {
      if (!single) {
        uint32_t rl = lo, rh = P.n_runs;
        while (rh - rl > 1) {
          const uint32_t mid = rl + ((rh - rl) >> 1);
          if (P.run_vstart[mid] <= j_lane)
            rl = mid;
          else
            rh = mid;
        }
        run = rl;
      }
      const uint64_t rv0 = single ? v0 : P.run_vstart[run], rv1 = single ? v1 : P.run_vstart[run + 1];
      const uint64_t xo = P.run_pos[run] + (j_lane - rv0); // outgoing bases xo .. xo+63, incoming bases xo+k .. xo+k+63
      if (n_mine == SEL_PER_LANE && j_lane + SEL_PER_LANE <= rv1) {
        // both base streams of the lane as four aligned words each, in registers: no LDS traffic for bases.  Per
        // 16 steps the two words are woven into two words of 4-bit (incoming, outgoing) pairs -- even steps and odd
        // steps -- so that a step forms its roll-table offset with one shift and one mask.
        const uint32_t sh_o = 2u * ((uint32_t)xo & 15u), sh_i = 2u * ((uint32_t)(xo + k) & 15u);
        const uint32_t* wo = P.pack + (xo >> 4);
        const uint32_t* wi = P.pack + ((xo + k) >> 4);
        uint32_t ro[5], ri[5], O[4], I[4];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
          ro[q] = wo[q];
          ri[q] = wi[q];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          O[q] = __builtin_amdgcn_alignbit(ro[q + 1], ro[q], sh_o);
          I[q] = __builtin_amdgcn_alignbit(ri[q + 1], ri[q], sh_i);
        }
        // the lane's first k-mer: its bases are the head of the outgoing stream
        if (k <= 64)
          hash_init_packed(P.hp, O, f, r);
        else
          hash_init(P.hp, [&](uint32_t i) { return base_abs(xo + i); }, f, r);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          // make room before a block of 16 steps if it could run out (one batch of probes per block at most)
          if ((cur >> 11) > P.flush_at && (cur >> 11) > acc) flush();
          const uint32_t even = (O[q] & 0x33333333u) | ((I[q] & 0x33333333u) << 2);
          const uint32_t odd = ((O[q] >> 2) & 0x33333333u) | (I[q] & 0xCCCCCCCCu);
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const uint32_t pairs = (j & 1) ? odd : even;
            const int sh = 4 * (j >> 1) - 3;
            step((sh < 0 ? pairs << 3 : pairs >> sh) & 0x78u, 16u * q + j);
          }
        }
      } else {
        shared_lane = true;
      }
    }
    // Lanes whose 64 k-mers are not one stretch of one run (a run boundary inside, or the end of the tile) are taken by
    // the whole wave, one after the other: lane l hashes the owner's k-mer number l from scratch (its own run looked up
    // from the owner's), the hits are ranked by a ballot and go to the owner's slots in order, and the owner books them.
    // A boundary costs the wave a few hundred instructions this way; rolling the 64 k-mers alone took ten times that.
    {
      const uint32_t lane = tid & 63u;
      unsigned long long todo = __ballot(shared_lane);
      while (todo) {
        const uint32_t o = (uint32_t)__ffsll((long long)todo) - 1u;
        todo &= todo - 1ULL;
        const uint64_t jo = __shfl(j_lane, (int)o, 64);
        const uint32_t nm = __shfl(n_mine, (int)o, 64);
        const uint32_t run_o = __shfl(run, (int)o, 64);
        const uint32_t cur_o = __shfl(cur, (int)o, 64);
        bool hit = false;
        uint64_t h = 0;
        if (lane < nm) {
          const uint64_t j = jo + lane;
          uint32_t rr = run_o;
          while (P.run_vstart[rr + 1] <= j) ++rr; // (j < n_valid = run_vstart[n_runs])
          const uint64_t s0 = P.run_pos[rr] + (j - P.run_vstart[rr]);
          uint64_t hf = 0, hr = 0;
          hash_init(P.hp, [&](uint32_t i) { return base_abs(s0 + i); }, hf, hr);
          h = hf + hr;
          hit = (uint32_t)(h >> 32) <= tau_hi;
        }
        const unsigned long long hm = __ballot(hit);
        if (hit) {
          const uint32_t rank = (uint32_t)__popcll(hm & ((1ULL << lane) - 1ULL));
          const uint32_t spare_o = SEL_SLOTS * ROW + (tid - lane + o) * 8u;
          *reinterpret_cast<uint64_t*>(ch_bytes + min(cur_o + rank * ROW, spare_o)) = h;
        }
        if (lane == o) {
          cur += (uint32_t)__popcll(hm) * ROW;
          pen_lo |= (uint32_t)hm;
          pen_hi |= (uint32_t)(hm >> 32);
        }
      }
    }
    if (!over) flush(); // what the lane parked last (or the overflow, if that is what happened)
    if (!__syncthreads_or(over)) {
      // every slot in use now holds an accepted candidate, in index order
      static_assert(SEL_SLOTS * HASH_THREADS >= SEL_CAP, "the general path stages SEL_CAP candidates in the same arrays");
      uint32_t accepted = 0;
      const uint32_t off = block_excl_scan_256(acc, s_w, &accepted);
      if (tid == 0) {
        s_base = accepted ? atomicAdd(&P.seg_count[seg], (unsigned long long)accepted) : 0ULL;
        P.tile_off[tile] = s_base;
        P.tile_cnt[tile] = accepted;
        P.tile_ordered[tile] = 1;
      }
      __syncthreads();
      const uint64_t base = s_base;
      if (accepted == 0 || base + accepted > P.seg_cap) return; // overflow: the host sees the counter and retries
      uint64_t* dj = P.seg_j + (uint64_t)seg * P.seg_cap + base + off;
      uint64_t* dk = P.seg_key + (uint64_t)seg * P.seg_cap + base + off;
      for (uint32_t i = 0; i < acc; ++i) {
        dj[i] = J0 + first + (uint32_t)__builtin_ctzll(acc_mask);
        acc_mask &= acc_mask - 1;
        dk[i] = s_ch[i * HASH_THREADS + tid];
      }
      return;
    }
    // some lane ran out of slots: redo the tile on the general path (the slots are simply overwritten)
  }
  if (tid == 0) P.tile_ordered[tile] = 0;
  roll_pass(0, SEL_TILE);
  __syncthreads();
  const uint32_t total = s_ctl[0];
  if (total <= SEL_CAP) {
    uint32_t mine = 0, accepted = 0;
    const uint32_t bits = probe_staged(total, &mine);
    (void)block_excl_scan_256(mine, s_w, &accepted);
    if (tid == 0) {
      s_base = accepted ? atomicAdd(&P.seg_count[seg], (unsigned long long)accepted) : 0ULL;
      P.tile_off[tile] = s_base;
      P.tile_cnt[tile] = accepted;
    }
    __syncthreads();
    const uint64_t base = s_base;
    if (accepted == 0 || base + accepted > P.seg_cap) return; // overflow: the host sees the counter and retries
    write_staged(total, bits, (uint64_t)seg * P.seg_cap + base);
    return;
  }
  // ---- overflow: 8 index ranges of 2048, counted first, then written in range order ------------------------
  constexpr uint32_t RANGE = 2048;
  uint32_t accepted = 0;
  for (uint32_t r0 = 0; r0 < SEL_TILE; r0 += RANGE) {
    __syncthreads();
    if (tid == 0) s_ctl[0] = 0;
    __syncthreads();
    roll_pass(r0, r0 + RANGE);
    __syncthreads();
    uint32_t mine = 0, acc = 0;
    (void)probe_staged(s_ctl[0], &mine);
    (void)block_excl_scan_256(mine, s_w, &acc);
    accepted += acc;
  }
  if (tid == 0) {
    s_base = accepted ? atomicAdd(&P.seg_count[seg], (unsigned long long)accepted) : 0ULL;
    P.tile_off[tile] = s_base;
    P.tile_cnt[tile] = accepted;
    s_ctl[1] = 0;
  }
  __syncthreads();
  const uint64_t base = s_base;
  if (accepted == 0 || base + accepted > P.seg_cap) return;
  for (uint32_t r0 = 0; r0 < SEL_TILE; r0 += RANGE) {
    __syncthreads();
    if (tid == 0) s_ctl[0] = 0;
    __syncthreads();
    roll_pass(r0, r0 + RANGE);
    __syncthreads();
    uint32_t mine = 0;
    const uint32_t n = s_ctl[0];
    const uint32_t bits = probe_staged(n, &mine);
    write_staged(n, bits, (uint64_t)seg * P.seg_cap + base); // s_ctl[1] keeps advancing: ranges land in order
  }
}

// ---- k_hash_select_hi: the same selection, rolling only the upper 31 bits of the two strand hashes -------------------------
// srol1/sror1 rotate bits 33..63 among themselves, so the upper 31 bits of the forward and of the reverse hash are rolling
// hashes of their own, and  (h0 >> 33)  is  (fH + rH) mod 2^31  or that plus one (the carry out of the lower 33 bits).
// A k-mer can only be a candidate (h0 <= tau) if  (fH + rH) mod 2^31 <= (tau >> 33)  or the sum is all ones; that test costs
// 11 instructions per k-mer on 32-bit registers instead of 21 on register pairs:
//   * a 31-bit value x is held as W = (x << 1) | (x >> 30), i.e. with its top bit repeated in bit 0; then
//       rotl31:  W' = alignbit(W, W << 1, 31)      rotr31:  W' = alignbit(W >> 1, W, 1)        (two instructions each)
//     and XOR keeps the form.  Wf + Wr + 2 (mod 2^32) lies in [2S + 2, 2S + 4] for S = (fH + rH) mod 2^31, so
//     "Wf + Wr + 2 <= 2 (tau >> 33) + 4" passes every k-mer with S <= tau >> 33 and S = 2^31 - 1 (which wraps to 0..2).
//   * the pass/fail bit of a step is shifted into the lane's mask with the carry-in of one add (v_addc).
// The ~c/w of the k-mers that pass (plus every k-mer of a lane whose 64 k-mers are not one stretch of one run) are listed in
// index order; the listed k-mers are then hashed in full, ceil(k/4) reads of the 4-bases-at-a-time table in LDS per k-mer
// with every lane busy, put to the exact test h0 <= tau, probed in the filter, and the accepted ones written in order.
//
// With the rolling this cheap the kernel is bound by the latency of those probes (random HBM reads) unless they overlap
// the rolling, so: a WAVE is the unit of work (tile = 4096 indices, no workgroup barriers; the waves of a workgroup only
// share the table), and each wave takes several consecutive tiles in a software pipeline -- the probes of tile t are in
// flight while tile t+1 is rolled.  Memory operations retire in issue order, so the base words of tile t+1 are requested
// BEFORE the probes of tile t, and the probes are issued unconditionally (a fixed count per lane; an unused slot reads
// word 0), which lets the wait before the rolling leave exactly the probes outstanding.
// Same outputs as k_hash_select with 4096-index tiles; its lists are always ordered.  For k <= 32 (the table is 4 KiB per
// four bases) and tau below half the hash range; the host launches k_hash_select otherwise.
constexpr uint32_t HIW_TILE = 64 * SEL_PER_LANE; // 4096 indices per wave tile
constexpr uint32_t HIW_WAVES = 8;                // waves per workgroup (they share the table; no barriers after the load)
constexpr uint32_t HIW_THREADS = 64 * HIW_WAVES;
constexpr uint32_t HIW_PER_MAX = 4;              // listed k-mers per lane and round: template parameter, 2 or 4
                                                 // (a tile has ~4096 c/w of them: 75 at c = 18, w = 1000)
constexpr uint32_t HI_K_MAX = 32;

__device__ __forceinline__ uint32_t hi_wform(uint64_t h)
{
  const uint32_t hi = (uint32_t)(h >> 32);
  return (hi & ~1u) | (hi >> 31);
}

// one 64-bit word through the scalar cache (wave-uniform address).  Written out because the compiler only uses scalar loads
// for memory it can prove nothing writes, and these tables sit behind plain pointers next to the kernel's outputs; as vector
// loads they would also queue up with the loads the pipeline below counts.
__device__ __forceinline__ uint64_t sload64(const uint64_t* p, uint32_t idx)
{
  uint64_t v;
  asm volatile("s_load_dwordx2 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=&s"(v) : "s"(p), "s"(idx * 8u) : "memory");
  return v;
}

// exclusive prefix sum over the 64 lanes of a wave + total, for small counts (v <= 64): one ballot per bit of the count
// (three for the usual 0..7, four more only if some lane holds 8 or more) -- no cross-lane data movement, no LDS latency
__device__ __forceinline__ uint32_t wave_excl_scan_small(uint32_t v, uint64_t below, uint32_t* total)
{
  uint32_t pre = 0, tot = 0;
#pragma unroll
  for (uint32_t b = 0; b < 3; ++b) {
    const unsigned long long m = __ballot((v >> b) & 1u);
    pre += (uint32_t)__popcll(m & below) << b;
    tot += (uint32_t)__popcll(m) << b;
  }
  if (__ballot(v >> 3) != 0ULL) {
#pragma unroll
    for (uint32_t b = 3; b < 7; ++b) {
      const unsigned long long m = __ballot((v >> b) & 1u);
      pre += (uint32_t)__popcll(m & below) << b;
      tot += (uint32_t)__popcll(m) << b;
    }
  }
  *total = tot;
  return pre;
}

// 64 rolling steps on the upper words; ro/ri = the five base words holding the lane's outgoing / incoming streams
__device__ __forceinline__ void hi_roll64(const uint32_t (&ro)[5], const uint32_t (&ri)[5], uint32_t sh_o, uint32_t sh_i, const ulonglong2* s_T,
                                          const uint2* s_roll, uint32_t nch, uint32_t limit, uint32_t& pen0, uint32_t& pen1)
{
  uint32_t O[4], I[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    O[q] = __builtin_amdgcn_alignbit(ro[q + 1], ro[q], sh_o);
    I[q] = __builtin_amdgcn_alignbit(ri[q + 1], ri[q], sh_i);
  }
  // upper words of the lane's first k-mer: its bases are the head of the outgoing stream
  uint32_t wf = 0, wr = 0;
#pragma unroll
  for (uint32_t c = 0; c < HI_K_MAX / 4; ++c) {
    if (c < nch) {
      const ulonglong2 e = s_T[c * 256u + ((O[c >> 2] >> (8u * (c & 3u))) & 255u)];
      wf ^= (uint32_t)(e.x >> 32);
      wr ^= (uint32_t)(e.y >> 32);
    }
  }
  wf = (wf & ~1u) | (wf >> 31);
  wr = (wr & ~1u) | (wr >> 31);
  const uint8_t* const roll_bytes = reinterpret_cast<const uint8_t*>(s_roll);
  pen0 = pen1 = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t even = (O[q] & 0x33333333u) | ((I[q] & 0x33333333u) << 2);
    const uint32_t odd = ((O[q] >> 2) & 0x33333333u) | (I[q] & 0xCCCCCCCCu);
    uint32_t pen = 0;
    // the table reads of eight steps are requested together (their addresses depend on the bases alone), then the eight
    // dependent steps run: with one read per 11-instruction step requested a step ahead, the wave waited for LDS every step
#pragma unroll
    for (int j0 = 0; j0 < 16; j0 += 8) {
      uint2 tb[8];
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int j = j0 + jj;
        const uint32_t pairs = (j & 1) ? odd : even;
        const int sh = 4 * (j >> 1) - 3;
        const uint32_t t8 = (sh < 0 ? pairs << 3 : pairs >> sh) & 0x78u; // 8 * (4 * incoming + outgoing)
        tb[jj] = *reinterpret_cast<const uint2*>(roll_bytes + t8);
      }
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const uint32_t s = wf + wr + 2u;
        asm("v_cmp_ge_u32 vcc, %2, %1\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(pen) : "v"(s), "s"(limit) : "vcc");
        wf = __builtin_amdgcn_alignbit(wf, wf << 1, 31) ^ tb[jj].x;
        const uint32_t x = wr ^ tb[jj].y;
        wr = __builtin_amdgcn_alignbit(x >> 1, x, 1);
      }
    }
    // 16 steps shifted in from the right: step 16q+j sits at bit 15-j
    const uint32_t nat = __brev(pen) >> 16;
    if (q < 2)
      pen0 |= nat << (16 * q);
    else
      pen1 |= nat << (16 * (q - 2));
  }
}

// A lane of a tile that spans several runs (contig ends, N stretches): its own run is looked up; if its 64 k-mers are one
// stretch of that run they are rolled (base words straight from the image), else all of them are listed.
__device__ __forceinline__ uint2 hi_roll_multirun(const uint32_t* pack, const uint64_t* run_pos, const uint64_t* run_vstart, uint32_t n_runs,
                                               uint32_t run_lo, uint64_t j_lane, uint32_t n_mine, uint32_t k, const ulonglong2* s_T,
                                               const uint2* s_roll, uint32_t nch, uint32_t limit, bool& straddles)
{
  uint32_t rl = run_lo, rh = n_runs;
  while (rh - rl > 1) {
    const uint32_t mid = rl + ((rh - rl) >> 1);
    if (run_vstart[mid] <= j_lane)
      rl = mid;
    else
      rh = mid;
  }
  uint32_t pen0, pen1;
  straddles = false;
  if (n_mine == SEL_PER_LANE && j_lane + SEL_PER_LANE <= run_vstart[rl + 1]) {
    const uint64_t xo = run_pos[rl] + (j_lane - run_vstart[rl]);
    const uint32_t* wo = pack + (xo >> 4);
    const uint32_t* wi = pack + ((xo + k) >> 4);
    uint32_t ro[5], ri[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      ro[q] = wo[q];
      ri[q] = wi[q];
    }
    hi_roll64(ro, ri, 2u * ((uint32_t)xo & 15u), 2u * ((uint32_t)(xo + k) & 15u), s_T, s_roll, nch, limit, pen0, pen1);
  } else {
    // a run boundary among the lane's k-mers (or the genome's end): the wave hashes them together afterwards (k_hash_select_hi), one
    // k-mer per lane.  (Until round 5 all 64 were listed, which alone took a tile at a scaffold end or an N gap past the 128 entries
    // of its list and onto the two-sweep path: such tiles were ~20 times dearer than their neighbours.)
    pen0 = pen1 = 0;
    straddles = true;
  }
  return make_uint2(pen0, pen1);
}

// Output: a tile that lists at most 64 PER k-mers (all but the tiles in repeats and at run boundaries) writes its accepted
// k-mers into the slots of its wave at the head of the segment arrays (64 PER entries per tile, the wave's tiles one behind
// the other from [first tile * 64 PER ...) on) -- no counter to wait for; a tile with more reserves room behind the slots, in segment t % N_SEG, like k_hash_select does.  tile_off
// holds absolute offsets (all ones: the reservation did not fit, k_cand_compact raises the overflow flag).
//
// Memory operations of the pipeline, per wave and tile t (they retire in issue order; the counts below are what the
// explicit waits rely on):
//     [base words of tile t+1 -> LDS: 2 LDS-DMA loads]  [probes of tile t-1: PER loads]
//     wait until PER + 2 are outstanding: the base words of tile t (requested one tile earlier) are in LDS -> roll tile t
//     wait for all: probes of tile t-1 -> write its accepted k-mers
//     list tile t, hash the listed k-mers in full (bases from LDS) -> they wait for the next turn of the loop
// The loads are issued with explicit instructions: the probes land in registers that the compiler must not touch before
// the wait (they are requested and awaited within one turn, never across the loop edge, where it would be free to copy
// them), and its own bookkeeping of an LDS-DMA load makes every later load wait for everything.  Its waits for its own
// loads (the rare paths below) stay correct with these in the queue: a count it computes can only wait for more.
constexpr uint32_t HIW_STAGE_WORDS = 272; // 256 + 16: a tile's 4096 + k + alignment slack bases, 16 per word
constexpr uint32_t ELIM_REACH = 6;        // accepted neighbours looked at on either side when dropping candidates that cannot win

template <bool HAS_BF, uint32_t HIW_PER>
__global__ __launch_bounds__(HIW_THREADS) void k_hash_select_hi(SelParams P, uint32_t nch, uint32_t tpw, uint64_t n_tiles)
{
  constexpr uint32_t HIW_LIST = 64 * HIW_PER;
  static_assert(HIW_PER == 2 || HIW_PER == 4, "the waits count the probes");
  extern __shared__ __align__(16) uint8_t hi_dyn_lds[];
  ulonglong2* const s_T = reinterpret_cast<ulonglong2*>(hi_dyn_lds); // [nch][256] {forward, reverse} contributions of four bases
  __shared__ uint2 s_roll[16];
  __shared__ __align__(16) uint32_t s_stage[HIW_WAVES][2][HIW_STAGE_WORDS];
  __shared__ uint16_t s_lists[HIW_WAVES][HIW_LIST];
  __shared__ __align__(16) uint32_t s_probe[HIW_WAVES][HIW_PER][64]; // filter words of the probes in flight (LDS-DMA, one row per slot)
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6); // (uniform: everything derived from it stays in scalar registers)
  {
    const ulonglong2* src = reinterpret_cast<const ulonglong2*>(P.hp.init4);
    for (uint32_t i = tid; i < nch * 256u; i += HIW_THREADS) s_T[i] = src[i];
  }
  if (tid < 16) s_roll[tid] = make_uint2(hi_wform(P.hp.roll_f[tid]), hi_wform(P.hp.roll_r[tid]));
  __syncthreads(); // the only workgroup barrier
  uint16_t* const s_list = s_lists[wv];
  const uint32_t stage_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t*)(&s_stage[wv][0][0]);
  const uint32_t probe_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t*)(&s_probe[wv][0][0]);
  const uint32_t k = P.hp.k;
  const uint32_t tau_hi = (uint32_t)(P.tau >> 32);
  const uint32_t limit = 2u * (tau_hi >> 1) + 4u;
  const uint32_t key16_shift = 48u - (uint32_t)__builtin_clzll(P.tau | 0x10000ULL); // the 16 bits below the leading one of tau: keys are <= tau
  // Workgroups take the tile groups from both ends of the genome inwards (even ones from the front, odd ones from the back): an
  // assembly's tail of short scaffolds -- tiles in five or more pieces, each ~20 times dearer than a tile inside one run -- sits
  // at one end of the file, and in launch order the waves that get it started last and finished 0.9 ms after everybody else.
  const uint32_t blk = (blockIdx.x & 1u) ? gridDim.x - 1u - (blockIdx.x >> 1) : (blockIdx.x >> 1);
  const uint64_t tile_first = ((uint64_t)blk * HIW_WAVES + wv) * tpw;
  if (tile_first >= n_tiles) return;
  const uint32_t my_tiles = (uint32_t)min((uint64_t)tpw, n_tiles - tile_first);
  const uint32_t first = SEL_PER_LANE * lane;
  const uint64_t below = (1ULL << lane) - 1ULL;

  // geometry of a tile; the run holding its first index is carried from tile to tile.  (Plain variables, not a struct:
  // copying one from "next" to "current" went through scratch memory, i.e. through the queue the waits below count.)
  uint32_t run_next = 0;
  {
    const uint64_t J0 = tile_first * HIW_TILE;
    uint32_t lo = 0, hi = P.n_runs;
    while (hi - lo > 1) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (sload64(P.run_vstart, mid) <= J0)
        lo = mid;
      else
        hi = mid;
    }
    run_next = lo;
  }
  auto geometry = [&](uint64_t tile, uint64_t& J0, uint64_t& P0, uint32_t& len, uint32_t& run, uint32_t& single) {
    J0 = tile * HIW_TILE;
    len = (uint32_t)min((uint64_t)HIW_TILE, P.n_valid - J0);
    uint64_t v1 = sload64(P.run_vstart, run_next + 1);
    while (v1 <= J0) {
      ++run_next;
      v1 = sload64(P.run_vstart, run_next + 1);
    }
    run = run_next;
    single = J0 + len <= v1 ? 1u : 0u;
    P0 = sload64(P.run_pos, run_next) + (J0 - sload64(P.run_vstart, run_next));
  };
  // position of the k-mer with compact index j of a tile that spans several runs.  run_end: one past the run of the tile's last
  // index (set per tile, below) -- the searches of a tile's lanes run over the handful of runs the tile touches, not over the
  // run table from the tile's first run to its end: fifteen dependent loads per lane and per listed k-mer in an assembly of 25,000
  // runs, which made every tile at a scaffold end or an N gap ~20 times dearer than its neighbours (and the tail of short
  // scaffolds at the end of an assembly -- five boundaries per tile, the last tiles a wave takes -- the whole kernel 1.3 ms longer)
  uint32_t run_end = P.n_runs;
  auto position_of = [&](uint64_t j, uint32_t run_lo) -> uint64_t {
    uint32_t rl = run_lo, rh = run_end;
    while (rh - rl > 1) {
      const uint32_t mid = rl + ((rh - rl) >> 1);
      if (P.run_vstart[mid] <= j)
        rl = mid;
      else
        rh = mid;
    }
    return P.run_pos[rl] + (j - P.run_vstart[rl]);
  };
  // base words of a tile inside one run -> staging buffer `buf`: words [w0, w0 + 272) of the image, w0 = the word of its
  // first base rounded down to a multiple of four (16-byte source addresses); anything else: two loads all the same (the
  // waits count them), of the head of the image
  // (m0, the LDS address of an LDS-DMA load, is written inside the same asm statement that uses it.  It is not on the clobber lists:
  // m0 is a reserved register, the compiler ignores such a clobber -- and warned about it 28 times per build; the code object is
  // byte for byte the same with and without.  What keeps the compiler's own uses of m0 apart from these is checked on the ISA:
  // tests/test_kernel_isa_guard.py::test_select_hi_m0_is_only_ever_used_next_to_its_own_write.)
  auto stage_dma = [&](uint64_t t_P0, bool real, uint32_t buf) {
    const uint64_t w0 = real ? ((t_P0 >> 4) & ~3ULL) : 0ULL;
    const uint32_t lds = stage_lds + buf * (HIW_STAGE_WORDS * 4u);
    const uint32_t* ga = P.pack + w0 + 4u * lane;
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(ga), "s"(lds) : "memory");
    if (lane < 4) {
      const uint32_t* gb = ga + 256;
      asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gb), "s"(lds + 1024u) : "memory");
    }
  };
  // full hash of the k-mer whose first base is in word w (bit offset sh) of `words`
  auto full_hash = [&](const uint32_t* words, uint32_t sh) -> uint64_t {
    const uint32_t w0 = words[0], w1 = words[1], w2 = words[2];
    const uint32_t b_lo = __builtin_amdgcn_alignbit(w1, w0, sh), b_hi = __builtin_amdgcn_alignbit(w2, w1, sh);
    uint64_t f = 0, r = 0;
#pragma unroll
    for (uint32_t c = 0; c < HI_K_MAX / 4; ++c) {
      if (c < nch) {
        const ulonglong2 e = s_T[c * 256u + (((c < 4 ? b_lo : b_hi) >> (8u * (c & 3u))) & 255u)];
        f ^= e.x;
        r ^= e.y;
      }
    }
    return f + r;
  };

  // ---- the tile whose probes are requested at the top of the next turn ---------------------------------------------------------
  uint64_t pd_h[HIW_PER];
  uint32_t pd_i[HIW_PER], pd_w[HIW_PER], pd_b[HIW_PER];
  uint32_t pd_m = 0; // slots of this lane that hold a candidate
  uint64_t pd_tile = ~0ULL, pd_J0 = 0;
  uint32_t pd_single = 0; // the pending tile lies inside one run (hence one record)
#pragma unroll
  for (uint32_t i = 0; i < HIW_PER; ++i) {
    pd_h[i] = 0;
    pd_i[i] = 0;
    pd_w[i] = 0;
    pd_b[i] = 0;
  }
  auto issue_probes = [&]() {
    if (HAS_BF) {
      const uint32_t* wp[HIW_PER];
#pragma unroll
      for (uint32_t i = 0; i < HIW_PER; ++i) {
        const uint64_t bidx = P.fm(pd_h[i]);
        pd_b[i] = (uint32_t)bidx & 31u;
        wp[i] = P.bf + (((pd_m >> i) & 1u) ? (bidx >> 5) : 0ULL); // (an unused slot reads word 0: the count stays fixed)
      }
      // (into LDS, like the base words: a register that a load in flight has yet to fill must not be copied or spilled
      // before the wait, and nothing keeps the compiler from doing that during the rolling in between)
#pragma unroll
      for (uint32_t i = 0; i < HIW_PER; ++i)
        asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off" ::"v"(wp[i]), "s"(probe_lds + i * 256u) : "memory");
    }
  };
  auto wait_stage = [&]() { // the two LDS-DMA loads of the next tile and the probes stay in flight
    if (HAS_BF && HIW_PER == 4)
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if (HAS_BF)
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  };
  auto wait_probes = [&]() {
    if (HAS_BF) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
      for (uint32_t i = 0; i < HIW_PER; ++i) pd_w[i] = s_probe[wv][i][lane];
    }
  };
  // writes the accepted k-mers of the pending tile behind those of the wave's earlier tiles
  uint32_t wave_run = 0;
  auto finish_pending = [&]() {
    if (pd_tile == ~0ULL) return;
    uint32_t okm = pd_m;
    if (HAS_BF) {
#pragma unroll
      for (uint32_t i = 0; i < HIW_PER; ++i)
        if (!((pd_w[i] >> pd_b[i]) & 1u)) okm &= ~(1u << i);
    }
    // entries are dealt to the lanes in blocks of `per`: list order = lane-major
    uint32_t rank = 0, accepted = 0;
#pragma unroll
    for (uint32_t i = 0; i < HIW_PER; ++i) {
      const unsigned long long bm = __ballot((okm >> i) & 1u);
      rank += (uint32_t)__popcll(bm & below);
      accepted += (uint32_t)__popcll(bm);
    }
    // ---- accepted k-mers that cannot be the minimum of any window are dropped here ----------------------------------------------
    // An accepted k-mer e with an accepted L to its left (smaller key) and an accepted R to its right (smaller or equal key),
    // R - L <= w, is the rightmost minimum of no window: every window that holds e holds L or R.  Taking such a k-mer out of
    // the candidate list changes no window's minimum and no gap between candidates that spans a whole window (a window that
    // holds a candidate holds its own minimum, which stays) -- so everything behind this kernel sees a shorter list and
    // gives the same result.  Looked for among the ELIM_REACH accepted neighbours on either side, inside the tile (a tile
    // inside one run: one record), on the top 16 significant bits of the keys (a tie counts as "not smaller"): about two
    // thirds of the accepted k-mers at w = 1000.  The words of the probes, read above, make room for the packed entries.
    if (P.w_elim && pd_single && accepted > 2u && accepted + 2u * ELIM_REACH <= HIW_LIST) {
      // packed entries (key16 << 16) | index, ELIM_REACH all-ones words on either side of them: a neighbour beyond the list reads
      // as "not smaller" without a bounds check
      uint32_t* const s_e = &s_probe[wv][0][0];
      if (lane < 2u * ELIM_REACH) s_e[lane < ELIM_REACH ? lane : accepted + lane] = 0xFFFFFFFFu;
      uint32_t n = 0;
#pragma unroll
      for (uint32_t i = 0; i < HIW_PER; ++i) {
        if ((okm >> i) & 1u) {
          s_e[ELIM_REACH + rank + n] = ((uint32_t)(pd_h[i] >> key16_shift) << 16) | pd_i[i];
          ++n;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      // one entry per lane and pass (a tile rarely accepts more than 64); the verdicts travel back to the lanes that hold the
      // full keys as ballots.  Neighbours from the farthest to the nearest, each overwriting: the nearest smaller one stays.
      unsigned long long lost[HIW_PER];
#pragma unroll
      for (uint32_t ps = 0; ps < HIW_PER; ++ps) {
        lost[ps] = 0ULL;
        if (64u * ps < accepted) { // (uniform)
          const uint32_t* const me = s_e + ELIM_REACH + min(64u * ps + lane, accepted - 1u);
          const uint32_t floor16 = *me & 0xFFFF0000u; // a word below this has a smaller key16
          uint32_t wl = 0xFFFFFFFFu, wr = 0xFFFFFFFFu;
#pragma unroll
          for (int s1 = (int)ELIM_REACH; s1 >= 1; --s1) {
            const uint32_t L = me[-s1], R = me[s1];
            wl = L < floor16 ? L : wl;
            wr = R < floor16 ? R : wr;
          }
          const bool both = (wl & wr) != 0xFFFFFFFFu && wl != 0xFFFFFFFFu && wr != 0xFFFFFFFFu;
          lost[ps] = __ballot(64u * ps + lane < accepted && both && ((wr & 0xFFFFu) - (wl & 0xFFFFu) <= P.w_elim));
        }
      }
      uint32_t dead = 0; // this lane's entries that lose
#pragma unroll
      for (uint32_t i = 0; i < HIW_PER; ++i) {
        const uint32_t e = rank + (uint32_t)__popc(okm & ((1u << i) - 1u));
        unsigned long long m = lost[0];
#pragma unroll
        for (uint32_t ps = 1; ps < HIW_PER; ++ps) m = (e >> 6) == ps ? lost[ps] : m;
        if (((okm >> i) & 1u) && ((m >> (e & 63u)) & 1ULL)) dead |= 1u << i;
      }
      __builtin_amdgcn_wave_barrier(); // (the array is the landing place of the next probes)
      okm &= ~dead;
      rank = 0;
      accepted = 0;
#pragma unroll
      for (uint32_t i = 0; i < HIW_PER; ++i) {
        const unsigned long long bm = __ballot((okm >> i) & 1u);
        rank += (uint32_t)__popcll(bm & below);
        accepted += (uint32_t)__popcll(bm);
      }
    }
    // the wave's tiles write one after the other into the slots of the wave (tile_first ... + tpw): the lists of a wave end up
    // contiguous -- whole 128-byte lines for this kernel's stores and for the copy that follows, instead of a piece per tile
    const uint64_t list_at = tile_first * HIW_LIST + wave_run;
    const uint64_t dst = list_at + rank;
    wave_run += accepted;
    if (lane == 0) {
      P.tile_off[pd_tile] = list_at;
      P.tile_cnt[pd_tile] = accepted;
      P.tile_ordered[pd_tile] = 1;
    }
    uint32_t n = 0;
#pragma unroll
    for (uint32_t i = 0; i < HIW_PER; ++i) {
      if ((okm >> i) & 1u) {
        P.seg_j[dst + n] = pd_J0 + pd_i[i];
        P.seg_key[dst + n] = pd_h[i];
        ++n;
      }
    }
    pd_tile = ~0ULL;
    pd_m = 0;
  };

  struct
  {
    uint64_t J0, P0;
    uint32_t len, run;
    bool single;
  } g; // the tile being worked on (filled from the variables below at the top of each turn; never copied as a whole)
  uint64_t n_J0 = 0, n_P0 = 0;
  uint32_t n_len = 0, n_run = 0, n_single = 0;
  geometry(tile_first, n_J0, n_P0, n_len, n_run, n_single);
  stage_dma(n_P0, n_single != 0, 0);
  for (uint32_t t = 0; t < my_tiles; ++t) {
    const uint64_t tile = tile_first + t;
    const bool more = t + 1 < my_tiles;
    g.J0 = n_J0;
    g.P0 = n_P0;
    g.len = n_len;
    g.run = n_run;
    g.single = n_single != 0;
    run_end = g.run + 1u;
    if (!g.single) { // (uniform, through the scalar cache) the run of the tile's last index
      const uint64_t j_last = g.J0 + g.len - 1u;
      uint32_t lo = g.run, hi = (uint32_t)min((uint64_t)P.n_runs, (uint64_t)g.run + g.len);
      while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (sload64(P.run_vstart, mid) <= j_last)
          lo = mid;
        else
          hi = mid;
      }
      run_end = lo + 1u;
    }
    if (more) geometry(tile + 1, n_J0, n_P0, n_len, n_run, n_single);
    stage_dma(n_P0, more && n_single != 0, (t + 1) & 1u);
    issue_probes();
    wait_stage();
    const uint32_t* const st = s_stage[wv][t & 1u];
    const uint64_t w0 = (g.P0 >> 4) & ~3ULL; // (tile inside one run) the image word at st[0]
    const uint32_t n_mine = first < g.len ? min(SEL_PER_LANE, g.len - first) : 0u;
    // ---- roll: which of the lane's 64 k-mers can be candidates ---------------------------------------------------------------
    uint32_t pen0 = 0, pen1 = 0; // steps 0..31 / 32..63
    bool straddles = false;      // (tile in several runs) the lane's k-mers are not one stretch of one run
    if (n_mine) {
      if (g.single) {
        if (n_mine == SEL_PER_LANE) {
          const uint64_t xo = g.P0 + first;
          const uint32_t o_idx = (uint32_t)((xo >> 4) - w0), i_idx = (uint32_t)(((xo + k) >> 4) - w0);
          uint32_t ro[5], ri[5];
#pragma unroll
          for (int q = 0; q < 5; ++q) {
            ro[q] = st[o_idx + q];
            ri[q] = st[i_idx + q];
          }
          hi_roll64(ro, ri, 2u * ((uint32_t)xo & 15u), 2u * ((uint32_t)(xo + k) & 15u), s_T, s_roll, nch, limit, pen0, pen1);
        } else { // the end of the last tile: listed
          pen0 = n_mine >= 32 ? 0xFFFFFFFFu : ((1u << n_mine) - 1u);
          pen1 = n_mine <= 32 ? 0u : ((1u << (n_mine - 32)) - 1u);
        }
      } else {
        const uint2 pm = hi_roll_multirun(P.pack, P.run_pos, P.run_vstart, run_end, g.run, g.J0 + first, n_mine, k, s_T, s_roll, nch, limit, straddles);
        pen0 = pm.x;
        pen1 = pm.y;
      }
    }
    if (!g.single) { // (uniform) the lanes with a run boundary among their k-mers, one after the other: every lane of the wave hashes
                     // one of that lane's k-mers in full; the ones with h0 <= tau are its candidates (exactly, not a superset)
      unsigned long long todo = __ballot(straddles);
      while (todo) {
        const uint32_t o = (uint32_t)__ffsll((long long)todo) - 1u;
        todo &= todo - 1ULL;
        const uint32_t nm_o = (uint32_t)__shfl((int)n_mine, (int)o, 64);
        bool hit = false;
        if (lane < nm_o) {
          const uint64_t pp = position_of(g.J0 + SEL_PER_LANE * o + lane, g.run);
          hit = full_hash(P.pack + (pp >> 4), 2u * ((uint32_t)pp & 15u)) <= P.tau;
        }
        const unsigned long long hm = __ballot(hit);
        if (lane == o) {
          pen0 = (uint32_t)hm;
          pen1 = (uint32_t)(hm >> 32);
        }
      }
    }
    // ---- list this tile's k-mers, hash them in full ---------------------------------------------------------------------------
    const uint32_t cnt = (uint32_t)__popc(pen0) + (uint32_t)__popc(pen1);
    uint32_t C = 0;
    const uint32_t off = wave_excl_scan_small(cnt, below, &C);
    auto build_list = [&](uint32_t rb) {
      if (off + cnt > rb && off < rb + HIW_LIST) {
        uint32_t pos = off - rb; // may wrap below zero: those entries belong to an earlier round
        uint32_t a = pen0, b = pen1;
        while (a) {
          const uint32_t s1 = (uint32_t)__builtin_ctz(a);
          a &= a - 1u;
          if (pos < HIW_LIST) s_list[pos] = (uint16_t)(first + s1);
          ++pos;
        }
        while (b) {
          const uint32_t s1 = (uint32_t)__builtin_ctz(b);
          b &= b - 1u;
          if (pos < HIW_LIST) s_list[pos] = (uint16_t)(first + 32u + s1);
          ++pos;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    };
    // hashes of the entries [rb, rb + HIW_LIST) dealt to the lanes in blocks; returns the mask of this lane's candidates
    auto hash_round = [&](uint32_t rb, uint64_t (&h)[HIW_PER], uint32_t (&ix)[HIW_PER]) -> uint32_t {
      const uint32_t n = min(HIW_LIST, C - rb);
      const uint32_t per = (n + 63u) >> 6;
      const uint32_t e0 = lane * per;
      uint32_t m = 0;
#pragma unroll
      for (uint32_t i = 0; i < HIW_PER; ++i) {
        h[i] = 0;
        ix[i] = 0;
        if (i < per && e0 + i < n) {
          const uint32_t idx = s_list[e0 + i];
          ix[i] = idx;
          if (g.single) {
            const uint64_t p = g.P0 + idx;
            h[i] = full_hash(st + (uint32_t)((p >> 4) - w0), 2u * ((uint32_t)p & 15u));
          } else {
            const uint64_t p = position_of(g.J0 + idx, g.run);
            h[i] = full_hash(P.pack + (p >> 4), 2u * ((uint32_t)p & 15u));
          }
          if (h[i] <= P.tau) m |= 1u << i;
        }
      }
      __builtin_amdgcn_wave_barrier();
      return m;
    };
    if (C <= HIW_LIST) {
      build_list(0);
      uint64_t nh[HIW_PER];
      uint32_t ni[HIW_PER];
      const uint32_t nm = hash_round(0, nh, ni);
      // ---- the tile rolled before this one: its probes have had the roll and the listing to come back -------------------------
      wait_probes();
      finish_pending();
#pragma unroll
      for (uint32_t i = 0; i < HIW_PER; ++i) {
        pd_h[i] = nh[i];
        pd_i[i] = ni[i];
      }
      pd_m = nm;
      pd_tile = tile;
      pd_J0 = g.J0;
      pd_single = g.single ? 1u : 0u;
    } else {
      wait_probes();
      finish_pending();
      // many listed k-mers (repeats, a wide tau, a fragmented assembly -- every tile at a scaffold end or an N gap lists the 64 k-mers
      // of the lane that straddles it): first the k-mers with h0 <= tau are counted -- no probe: that many slots are reserved, an upper
      // bound --, then they are probed and the accepted ones written round by round.  (Round 3 probed in both sweeps: the first
      // sweep's blocking round trips to the filter were a third of such a tile's time.)
      const uint32_t seg = (uint32_t)(tile % N_SEG);
      uint32_t listed_ok = 0, accepted = 0;
      unsigned long long base = 0;
      bool fits = true;
      for (int sweep = 0; sweep < 2 && fits; ++sweep) {
        if (sweep == 1) {
          if (lane == 0) base = listed_ok ? atomicAdd(&P.seg_count[seg], (unsigned long long)listed_ok) : 0ULL;
          base = __shfl(base, 0, 64);
          fits = base + listed_ok <= P.seg_cap;
          if (listed_ok == 0 || !fits) break; // (overflow: the host sees the counter and retries)
        }
        uint64_t dst = n_tiles * HIW_LIST + (uint64_t)seg * P.seg_cap + base;
        for (uint32_t rb = 0; rb < C; rb += HIW_LIST) {
          build_list(rb);
          uint64_t h[HIW_PER];
          uint32_t ix[HIW_PER];
          uint32_t okm = hash_round(rb, h, ix);
          if (HAS_BF && sweep == 1) {
#pragma unroll
            for (uint32_t i = 0; i < HIW_PER; ++i)
              if (((okm >> i) & 1u) && !bf_test(P.bf, P.fm(h[i]))) okm &= ~(1u << i);
          }
          uint32_t rank = 0, acc = 0;
#pragma unroll
          for (uint32_t i = 0; i < HIW_PER; ++i) {
            const unsigned long long bm = __ballot((okm >> i) & 1u);
            rank += (uint32_t)__popcll(bm & below);
            acc += (uint32_t)__popcll(bm);
          }
          if (sweep == 0) {
            listed_ok += acc;
          } else {
            uint32_t n = 0;
#pragma unroll
            for (uint32_t i = 0; i < HIW_PER; ++i) {
              if ((okm >> i) & 1u) {
                P.seg_j[dst + rank + n] = g.J0 + ix[i];
                P.seg_key[dst + rank + n] = h[i];
                ++n;
              }
            }
            dst += acc;
            accepted += acc;
          }
        }
      }
      if (lane == 0) {
        P.tile_off[tile] = fits ? n_tiles * HIW_LIST + (uint64_t)seg * P.seg_cap + base : ~0ULL;
        P.tile_cnt[tile] = fits ? accepted : 0u;
        P.tile_ordered[tile] = 1;
      }
    }
  }
  issue_probes();
  wait_probes();
  finish_pending();
}

// Tile lists (scattered over the segments in completion order) -> one array ordered by compact index.  Lists of
// fast-path tiles are copied; for the others, per tile: counting sort by the lane that produced the entry (index / 64, 256 buckets: histogram,
// scan, scatter), then one lane per bucket orders the handful of entries it holds.  O(entries).
__global__ __launch_bounds__(256) void k_cand_compact(const uint64_t* __restrict__ seg_j, const uint64_t* __restrict__ seg_key,
                                                      uint64_t seg_cap, const uint64_t* __restrict__ tile_off,
                                                      const uint32_t* __restrict__ tile_cnt, const uint8_t* __restrict__ tile_ordered,
                                                      const uint64_t* __restrict__ out_off, uint64_t n_tiles, uint64_t* __restrict__ pj,
                                                      uint64_t* __restrict__ pk, uint64_t cap, unsigned long long* __restrict__ overflow,
                                                      bool absolute)
{
  // absolute: tile_off holds offsets into seg_j/seg_key as such (k_hash_select_hi), all ones = the tile's list was not written
  __shared__ uint64_t s_k[SEL_CAP];   // keys as read
  __shared__ uint64_t s_k2[SEL_CAP];  // keys in bucket order
  __shared__ uint16_t s_i[SEL_CAP];   // tile-local indices as read
  __shared__ uint16_t s_i2[SEL_CAP];
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_base[257];
  __shared__ uint32_t s_w[8];
  __shared__ uint32_t s_n;
  // A workgroup takes CC_TILES consecutive tiles.  Ordered lists (nearly all) are copied by 32 lanes each; the tiles
  // that need sorting are then taken one after the other by the whole workgroup.
  __shared__ uint32_t s_todo[CC_TILES];
  __shared__ uint32_t s_ntodo;
  if (threadIdx.x == 0) s_ntodo = 0;
  __syncthreads();
  {
    const uint64_t t = (uint64_t)blockIdx.x * CC_TILES + (threadIdx.x >> 5);
    const uint32_t l32 = threadIdx.x & 31u;
    if (t < n_tiles) {
      const uint32_t n = tile_cnt[t];
      // a tile whose list did not fit its segment was not written: the host retries with larger segments, and the
      // kernels after this one return at once (the candidate array has holes of stale data)
      const bool fits = absolute ? tile_off[t] != ~0ULL : tile_off[t] + n <= seg_cap;
      if (n != 0 && !fits && l32 == 0) *overflow = 1ULL;
      if (n != 0 && fits) {
        if (tile_ordered[t]) {
          const uint64_t src = absolute ? tile_off[t] : (t % N_SEG) * seg_cap + tile_off[t];
          const uint64_t dst = out_off[t];
          for (uint32_t e = l32; e < n; e += 32) {
            if (dst + e < cap) {
              pj[dst + e] = seg_j[src + e];
              pk[dst + e] = seg_key[src + e];
            }
          }
        } else if (l32 == 0) {
          s_todo[atomicAdd(&s_ntodo, 1u)] = (uint32_t)(threadIdx.x >> 5);
        }
      }
    }
  }
  __syncthreads();
  const uint32_t n_todo = s_ntodo;
  for (uint32_t td = 0; td < n_todo; ++td) {
  const uint64_t tile = (uint64_t)blockIdx.x * CC_TILES + s_todo[td];
  const uint32_t n = tile_cnt[tile];
  const uint64_t src = (tile % N_SEG) * seg_cap + tile_off[tile];
  uint64_t dst = out_off[tile];
  const uint64_t J0 = tile * SEL_TILE;
  const uint32_t n_ranges = n <= SEL_CAP ? 1u : SEL_TILE / 2048u;
  for (uint32_t r = 0; r < n_ranges; ++r) {
    const uint64_t lo = n_ranges == 1 ? J0 : J0 + 2048ull * r;
    const uint64_t hi = n_ranges == 1 ? J0 + SEL_TILE : lo + 2048ull;
    __syncthreads();
    if (threadIdx.x == 0) s_n = 0;
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
      const uint64_t j = seg_j[src + i];
      if (j >= lo && j < hi) {
        const uint32_t slot = atomicAdd(&s_n, 1u);
        if (slot < SEL_CAP) {
          const uint32_t idx = (uint32_t)(j - J0);
          s_i[slot] = (uint16_t)idx;
          s_k[slot] = seg_key[src + i];
          atomicAdd(&s_hist[idx >> 6], 1u);
        }
      }
    }
    __syncthreads();
    const uint32_t c = min(s_n, SEL_CAP);
    uint32_t tot = 0;
    const uint32_t mine = s_hist[threadIdx.x];
    const uint32_t base = block_excl_scan_256(mine, s_w, &tot);
    s_base[threadIdx.x] = base;
    if (threadIdx.x == 255) s_base[256] = base + mine;
    s_hist[threadIdx.x] = 0; // reused as the per-bucket fill cursor
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < c; e += 256) {
      const uint32_t b = s_i[e] >> 6;
      const uint32_t pos = s_base[b] + atomicAdd(&s_hist[b], 1u);
      s_i2[pos] = s_i[e];
      s_k2[pos] = s_k[e];
    }
    __syncthreads();
    { // lane b orders bucket b (insertion sort; a bucket holds at most 64 entries, typically 0-3)
      const uint32_t b0 = s_base[threadIdx.x], b1 = s_base[threadIdx.x + 1];
      for (uint32_t x = b0 + 1; x < b1; ++x) {
        const uint16_t vi = s_i2[x];
        const uint64_t vk = s_k2[x];
        uint32_t y = x;
        while (y > b0 && s_i2[y - 1] > vi) {
          s_i2[y] = s_i2[y - 1];
          s_k2[y] = s_k2[y - 1];
          --y;
        }
        s_i2[y] = vi;
        s_k2[y] = vk;
      }
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < c; e += 256) {
      if (dst + e < cap) {
        pj[dst + e] = J0 + s_i2[e];
        pk[dst + e] = s_k2[e];
      }
    }
    dst += c;
  }
  } // unordered tiles of this workgroup
}

// The same for the slots of k_hash_select_hi (every list ordered, at an absolute offset, at most a few hundred entries and
// typically ~60): sixteen lanes per tile, sixteen tiles per workgroup -- 128-byte pieces in and out, nothing else to do.
constexpr uint32_t CCS_TILES = 16;

__global__ __launch_bounds__(256) void k_cand_compact_slots(const uint64_t* __restrict__ seg_j, const uint64_t* __restrict__ seg_key,
                                                            const uint64_t* __restrict__ tile_off, const uint32_t* __restrict__ tile_cnt,
                                                            const uint64_t* __restrict__ out_off, uint64_t n_tiles, uint64_t* __restrict__ pj,
                                                            uint64_t* __restrict__ pk, uint64_t cap, unsigned long long* __restrict__ overflow)
{
  const uint64_t t = (uint64_t)blockIdx.x * CCS_TILES + (threadIdx.x >> 4);
  const uint32_t l16 = threadIdx.x & 15u;
  if (t >= n_tiles) return;
  // the three directory words together (one after the other they were three round trips before the first entry moved; entries
  // four rounds at a time with clamped indices made it slower, 0.10 -> 0.12 ms: a list holds ~25)
  const uint32_t n = tile_cnt[t];
  const uint64_t src = tile_off[t];
  const uint64_t dst = out_off[t];
  if (n == 0) return;
  if (src == ~0ULL) { // the tile's reservation did not fit: the host retries with larger segments
    if (l16 == 0) *overflow = 1ULL;
    return;
  }
  for (uint32_t e = l16; e < n; e += 16) {
    if (dst + e < cap) {
      pj[dst + e] = seg_j[src + e];
      pk[dst + e] = seg_key[src + e];
    }
  }
}

struct SparseParams
{
  const uint64_t* pj; // candidates: compact index, ascending
  const uint64_t* pk; //             key (h0 <= tau)
  const uint64_t* m_scan_last; // number of candidates = *m_scan_last + *m_cnt_last (device side: the host
  const uint32_t* m_cnt_last;  //   launches over the capacity m_max and never waits for the count)
  uint64_t m_max;
  const uint64_t* rec_vstart;
  const uint64_t* rec_nv;
  uint64_t n_valid; // = rec_vstart[n_rec - 1] + rec_nv[n_rec - 1]
  uint32_t n_rec;
  uint32_t w;
  uint64_t* stage_j; // winners of workgroup b, in order, at [b * SPARSE_BLOCK ...)
  uint64_t* stage_k;
  uint64_t* blk_cnt; // [grid] winners per workgroup (scanned afterwards => globally ordered output, no sort)
  uint64_t* gap_lo; // uncovered ranges [lo, hi] (inclusive), at least w long
  uint64_t* gap_hi;
  unsigned long long* gap_count;
  uint64_t gap_cap;
  const unsigned long long* overflow; // set by k_cand_compact: the candidate array is incomplete, do nothing
  uint32_t rec_holes = 0;             // 1: the records do not tile the index space (uncovered ranges as records): a record ends at rec_vstart + rec_nv
  uint32_t no_gaps = 0;               // 1: stretches without a candidate are not reported (accepted-list paths: nothing in them can be a minimizer) --
                                      // with w <= k every substitution leaves such a stretch, and reporting is an atomic on ONE counter each
};

__device__ __forceinline__ void push_gap(const SparseParams& P, uint64_t lo, uint64_t hi)
{
  const unsigned long long s = atomicAdd(P.gap_count, 1ULL);
  if (s < P.gap_cap) {
    P.gap_lo[s] = lo;
    P.gap_hi[s] = hi;
  }
}

constexpr uint32_t SPARSE_HALO = 64; // neighbours staged in LDS on each side; beyond that, global memory
constexpr uint32_t SPARSE_REC_LDS = 2048; // record tables up to this many records are searched in LDS

__global__ __launch_bounds__(SPARSE_THREADS) void k_sparse_win(SparseParams P)
{
  __shared__ uint32_t s_wcnt[SPARSE_THREADS / 64];
  __shared__ ulonglong2 s_c[SPARSE_BLOCK + 2 * SPARSE_HALO]; // staged candidates: x = compact index, y = key
  __shared__ uint64_t s_rv[SPARSE_REC_LDS];
  const uint64_t m = *P.overflow ? 0 : min(*P.m_scan_last + (uint64_t)*P.m_cnt_last, P.m_max);
  // records that hold no candidate at all are uncovered as a whole (no candidate of theirs will report them): a
  // binary search per record, spread over the launch (it used to be a kernel of its own on the critical path)
  if (!*P.overflow && !P.no_gaps)
    for (uint64_t r = (uint64_t)blockIdx.x * SPARSE_THREADS + threadIdx.x; r < P.n_rec; r += (uint64_t)gridDim.x * SPARSE_THREADS) {
      const uint64_t rs = P.rec_vstart[r], nv = P.rec_nv[r];
      if (nv < P.w) continue;
      uint64_t lo = 0, hi = m; // first candidate index >= rs
      while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (P.pj[mid] < rs)
          lo = mid + 1;
        else
          hi = mid;
      }
      if (lo >= m || P.pj[lo] >= rs + nv) push_gap(P, rs, rs + nv - 1);
    }
  if ((uint64_t)blockIdx.x * SPARSE_BLOCK >= m) {
    if (threadIdx.x == 0) P.blk_cnt[blockIdx.x] = 0;
    return;
  }
  // stage this workgroup's candidates and a halo: the neighbour scans below then run at LDS latency
  const uint64_t blk0 = (uint64_t)blockIdx.x * SPARSE_BLOCK;
  const uint64_t lds_lo = blk0 >= SPARSE_HALO ? blk0 - SPARSE_HALO : 0;
  const uint64_t lds_hi = min(m, blk0 + SPARSE_BLOCK + SPARSE_HALO);
  for (uint64_t q = lds_lo + threadIdx.x; q < lds_hi; q += SPARSE_THREADS) {
    s_c[q - lds_lo] = make_ulonglong2(P.pj[q], P.pk[q]);
  }
  // record starts: the per-candidate binary search below runs in LDS (a chain of dependent global loads otherwise)
  const bool recs_in_lds = P.n_rec <= SPARSE_REC_LDS && !P.rec_holes;
  if (recs_in_lds)
    for (uint32_t q = threadIdx.x; q < P.n_rec; q += SPARSE_THREADS) s_rv[q] = P.rec_vstart[q];
  __syncthreads();
  auto cand_j = [&](uint64_t q) -> uint64_t { return (q >= lds_lo && q < lds_hi) ? s_c[q - lds_lo].x : P.pj[q]; };
  auto cand_k = [&](uint64_t q) -> uint64_t { return (q >= lds_lo && q < lds_hi) ? s_c[q - lds_lo].y : P.pk[q]; };
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  uint32_t winners_so_far = 0;
  for (uint32_t item = 0; item < SPARSE_ITEMS; ++item) {
  const uint64_t i = blk0 + (uint64_t)item * SPARSE_THREADS + threadIdx.x;
  bool win = false;
  uint64_t j = 0, key = 0;
  if (i < m) {
    j = cand_j(i);
    key = cand_k(i);
    uint32_t lo = 0, hi = P.n_rec;
    if (recs_in_lds) {
      while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (s_rv[mid] <= j)
          lo = mid;
        else
          hi = mid;
      }
    } else {
      while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (P.rec_vstart[mid] <= j)
          lo = mid;
        else
          hi = mid;
      }
    }
    // records may have zero valid k-mers (equal vstart): take the last record starting at or before j.  Its compact
    // indices end where the next record's start (the index space has no holes).
    uint64_t rs, re;
    if (recs_in_lds) {
      rs = s_rv[lo];
      re = lo + 1 < P.n_rec ? s_rv[lo + 1] : P.n_valid;
    } else {
      rs = P.rec_vstart[lo];
      re = rs + P.rec_nv[lo];
    }
    const uint64_t w = P.w;
    if (re - rs >= w) {
      // Nearest strictly smaller key to the left / smaller-or-equal key to the right, within the window reach and
      // the record.  The scans run over the staged candidates only (tight loops: two LDS reads and two compares per
      // step); a lane whose scan leaves the staged range while still inside its reach -- more than SPARSE_HALO
      // candidates within w k-mers -- repeats it through global memory.
      const uint64_t a_lim = (j - rs >= w - 1) ? j - (w - 1) : rs;
      const uint64_t b_lim = (re - 1 - j >= w - 1) ? j + (w - 1) : re - 1;
      uint64_t a_min = a_lim, b_max = b_lim;
      const uint32_t li = (uint32_t)(i - lds_lo), n_st = (uint32_t)(lds_hi - lds_lo);
      bool redo_left = lds_lo > 0, redo_right = lds_hi < m;
      // both directions in one loop, one 16-byte LDS read per direction and step, the exits as predicates: the loop
      // control is then a handful of scalar instructions per step (with two loops of two breaks each, the scalar unit
      // -- exec-mask bookkeeping -- was what the kernel waited for)
      {
        // cursor per direction; a scan that met its stop condition keeps the index where it stopped and sets the top
        // bit (neither active any more, nor "ran off the staged range", which is what asks for the pass through global
        // memory); what the stop means for a_min / b_max is worked out once, after the loop
        constexpr uint32_t STOPPED = 0x80000000u;
        uint32_t ql = li, qr = li;
        for (;;) {
          const bool gl = ql - 1u < STOPPED - 1u; // 0 < ql, not stopped
          const bool gr = qr + 1u < n_st;         // (a stopped cursor + 1 is not below n_st)
          if (!(gl | gr)) break;
          const uint32_t il = ql - (gl ? 1u : 0u), ir = qr + (gr ? 1u : 0u);
          const ulonglong2 L = s_c[min(il, n_st - 1u)], R = s_c[min(ir, n_st - 1u)]; // (a parked cursor reads a valid entry)
          ql = (gl & ((L.x < a_lim) | (L.y < key))) ? (il | STOPPED) : il;
          qr = (gr & ((R.x > b_lim) | (R.y <= key))) ? (ir | STOPPED) : ir;
        }
        if (ql & STOPPED) { // left: by a smaller key inside the reach, or by leaving the reach
          const uint64_t x = s_c[ql & ~STOPPED].x;
          if (x >= a_lim) a_min = x + 1;
        }
        if (qr & STOPPED) {
          const uint64_t x = s_c[qr & ~STOPPED].x;
          if (x <= b_lim) b_max = x - 1;
        }
        redo_left = redo_left & (ql == 0u);
        redo_right = redo_right & (qr + 1u == n_st);
      }
      if (redo_left) {
        a_min = a_lim;
        for (uint64_t q = i; q-- > 0;) {
          const uint64_t jq = cand_j(q);
          if (jq < a_lim) break;
          if (cand_k(q) < key) {
            a_min = jq + 1;
            break;
          }
        }
      }
      if (redo_right) {
        b_max = b_lim;
        for (uint64_t q = i + 1; q < m; ++q) {
          const uint64_t jq = cand_j(q);
          if (jq > b_lim) break;
          if (cand_k(q) <= key) {
            b_max = jq - 1;
            break;
          }
        }
      }
      bool have_next = false;
      uint64_t j_next = 0;
      if (i + 1 < m) { // (i + 1 < m <=> li + 1 < n_st: the halo, or the end of the list)
        j_next = s_c[li + 1].x;
        have_next = j_next < re;
      }
      win = b_max - a_min + 1 >= w;
      // uncovered ranges: to the next candidate of the record (or the record end), and before the first
      const uint64_t nxt = have_next ? j_next : re; // first index after the gap
      if (!P.no_gaps) {
        if (nxt - j - 1 >= w) push_gap(P, j + 1, nxt - 1);
        const bool first_in_rec = (i == 0) || (s_c[li - 1].x < rs); // (i > 0 => li > 0)
        if (first_in_rec && j - rs >= w) push_gap(P, rs, j - 1);
      }
    }
  }
  // ordered compaction: candidates are in index order across lanes, waves, rounds and workgroups
  const unsigned long long bal = __ballot(win);
  if (item) __syncthreads(); // (the counts of the round before have been read)
  if (lane == 0) s_wcnt[wv] = (uint32_t)__popcll(bal);
  __syncthreads();
  uint32_t base = 0, total = 0;
  for (uint32_t q = 0; q < SPARSE_THREADS / 64; ++q) {
    const uint32_t c = s_wcnt[q];
    if (q < wv) base += c;
    total += c;
  }
  if (win) {
    const uint32_t r = winners_so_far + base + (uint32_t)__popcll(bal & ((1ULL << lane) - 1ULL));
    P.stage_j[blk0 + r] = j;
    P.stage_k[blk0 + r] = key;
  }
  winners_so_far += total;
  } // items
  if (threadIdx.x == 0) P.blk_cnt[blockIdx.x] = winners_so_far;
}

// per-workgroup winner lists -> one ordered array
__global__ __launch_bounds__(256) void k_gather_winners(const uint64_t* __restrict__ stage_j, const uint64_t* __restrict__ stage_k,
                                                       const uint64_t* __restrict__ blk_cnt, const uint64_t* __restrict__ blk_scan,
                                                       uint64_t* __restrict__ out_j, uint64_t* __restrict__ out_k)
{
  const uint64_t b = blockIdx.x;
  const uint64_t n = blk_cnt[b], dst = blk_scan[b], src = b * SPARSE_BLOCK;
  for (uint64_t i = threadIdx.x; i < n; i += 256) {
    out_j[dst + i] = stage_j[src + i];
    out_k[dst + i] = stage_k[src + i];
  }
}

// merge a short sorted list into a long sorted one (disjoint keys): every element finds its final slot
__global__ __launch_bounds__(256) void k_merge_lists(const uint64_t* __restrict__ a_j, const uint64_t* __restrict__ a_k, uint64_t na,
                                                    const uint64_t* __restrict__ b_j, const uint64_t* __restrict__ b_k, uint64_t nb,
                                                    uint64_t* __restrict__ out_j, uint64_t* __restrict__ out_k)
{
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= na + nb) return;
  const bool from_a = t < na;
  const uint64_t self = from_a ? t : t - na;
  const uint64_t key = from_a ? a_j[self] : b_j[self];
  const uint64_t* other = from_a ? b_j : a_j;
  uint64_t lo = 0, hi = from_a ? nb : na;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (other[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  out_j[self + lo] = key;
  out_k[self + lo] = from_a ? a_k[self] : b_k[self];
}

// ---- few uncovered ranges: their winners are strung together and merged without going back to the host ------------
// k_gap_collect (one workgroup): per-tile winner lists of the window kernel (each in index order, tiles in index order)
// -> one list; ctl[0] = their number, ctl[1] = sparse + dense winners, ctl[2] = 1 if they do not fit (a tile with more
// than GAP_TILE_CAP winners, or more than GAP_LIST_CAP in all): the host then repeats the call on the general path.
constexpr uint32_t GAP_TILE_CAP = 128;   // winners per window tile (4096 windows: about 8 at w = 1000)
constexpr uint32_t GAP_TILES_MAX = 4096; // window tiles handled this way
constexpr uint32_t GAP_LIST_CAP = 65536; // winners in all (a family with insertions of tens of kbp: ~1500 ranges, ~6000 winners at 3 Gbp)
constexpr uint32_t GAP_COLLECT_THREADS = 1024;

__global__ __launch_bounds__(GAP_COLLECT_THREADS) void k_gap_collect(const uint32_t* __restrict__ tile_cnt, uint32_t n_tiles,
                                                                     const uint64_t* __restrict__ tile_j,
                                                                     const uint64_t* __restrict__ tile_key, uint64_t n_sparse,
                                                                     uint64_t* __restrict__ out_j, uint64_t* __restrict__ out_key,
                                                                     uint64_t* __restrict__ ctl)
{
  static_assert(GAP_TILES_MAX == 4 * GAP_COLLECT_THREADS, "four tiles per lane");
  __shared__ uint32_t s_off[GAP_TILES_MAX + 1];
  __shared__ uint32_t s_wave[GAP_COLLECT_THREADS / 64];
  __shared__ uint32_t s_bad;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  if (tid == 0) s_bad = 0;
  uint32_t c[4], sum = 0;
  bool bad = false;
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {
    const uint32_t t = 4u * tid + q;
    c[q] = t < n_tiles ? tile_cnt[t] : 0u;
    bad |= c[q] > GAP_TILE_CAP;
    c[q] = min(c[q], GAP_TILE_CAP);
    sum += c[q];
  }
  uint32_t inc = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(inc, d, 64);
    if ((int)lane >= d) inc += up;
  }
  if (lane == 63) s_wave[wv] = inc;
  __syncthreads();
  if (bad) s_bad = 1;
  uint32_t before = inc - sum;
  for (uint32_t x = 0; x < wv; ++x) before += s_wave[x];
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {
    s_off[4u * tid + q] = before;
    before += c[q];
  }
  if (tid == GAP_COLLECT_THREADS - 1) s_off[GAP_TILES_MAX] = before;
  __syncthreads();
  const uint32_t n = s_off[GAP_TILES_MAX];
  if (s_bad || n > GAP_LIST_CAP) {
    if (tid == 0) {
      ctl[0] = 0;
      ctl[1] = n_sparse;
      ctl[2] = 1;
    }
    return;
  }
  for (uint32_t e = tid; e < n; e += GAP_COLLECT_THREADS) {
    uint32_t lo = 0, hi = GAP_TILES_MAX; // last tile whose offset is <= e (empty tiles share an offset: take the last)
    while (hi - lo > 1) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (s_off[mid] <= e)
        lo = mid;
      else
        hi = mid;
    }
    const uint64_t src = (uint64_t)lo * GAP_TILE_CAP + (e - s_off[lo]);
    out_j[e] = tile_j[src];
    out_key[e] = tile_key[src];
  }
  if (tid == 0) {
    ctl[0] = n;
    ctl[1] = n_sparse + n;
    ctl[2] = 0;
  }
}


// ---- sparse filters: the accepted k-mers themselves as the candidate list --------------------------------------------------
// When the common filter is all but empty (occupancy x summary granule << 1), every k-mer can afford a look at the filter's
// L2-resident summary, and the few that pass it and the filter ARE the candidates (tau = everything): the windows are then
// decided among accepted k-mers alone by k_sparse_win, and a window without one has no minimizer -- no keys, no window
// kernel, no uncovered ranges.  Output format of k_hash_select: per-tile lists in index order (tile = 8192 k-mers here).
struct AcceptParams
{
  const uint8_t* code;
  const uint64_t* run_pos;
  const uint64_t* run_vstart;
  uint32_t n_runs;
  uint64_t n_valid;
  HashParams hp;
  const uint32_t* bf;
  FastMod fm;
  const uint32_t* summary;
  uint32_t shift;
  uint32_t probe_mask; // all ones; a measurement can clear it (NTS_ACC_NO_LOOKUP=1: nothing passes the folded copy -- wrong results, the
                       // kernel's time without its L2 and HBM lookups)
  uint64_t* seg_j;
  uint64_t* seg_key;
  uint64_t seg_cap;
  unsigned long long* seg_count;
  uint64_t* tile_off;
  uint32_t* tile_cnt;
  uint8_t* tile_ordered;
};

__global__ __launch_bounds__(HASH_THREADS) void k_hash_accept(AcceptParams P)
{
  __shared__ uint64_t s_tab[36];
  __shared__ uint32_t s_seq[SEQ_LDS_DWORDS];
  __shared__ uint32_t s_w[8];
  __shared__ unsigned long long s_base;
  const uint32_t tid = threadIdx.x;
  if (tid < 16) {
    s_tab[tid] = P.hp.roll_f[tid];
    s_tab[16 + tid] = P.hp.roll_r[tid];
  }
  if (tid < 4) s_tab[32 + tid] = P.hp.seed[tid];
  const uint32_t k = P.hp.k;
  const uint64_t tile = blockIdx.x;
  const uint64_t J0 = tile * KEY_TILE;
  const uint32_t tile_len = (uint32_t)min((uint64_t)KEY_TILE, P.n_valid - J0);
  uint32_t lo = 0, hi = P.n_runs;
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (P.run_vstart[mid] <= J0)
      lo = mid;
    else
      hi = mid;
  }
  const uint64_t v0 = P.run_vstart[lo], v1 = P.run_vstart[lo + 1];
  const bool single = (J0 + tile_len <= v1) && (k <= FAST_K_MAX);
  const uint32_t first = 32u * tid;
  const uint32_t n_mine = first < tile_len ? min(32u, tile_len - first) : 0u;
  uint32_t acc_mask = 0, n_acc = 0;
  uint64_t acc_h[4] = { 0, 0, 0, 0 };
  auto accepted = [&](uint64_t h) -> bool {
    const uint64_t idx = P.fm(h);
    const uint64_t g = idx >> P.shift;
    if (!((P.summary[g >> 5] >> (g & 31u)) & 1u)) return false;
    return (P.bf[idx >> 5] >> ((uint32_t)idx & 31u)) & 1u;
  };
  const uint8_t* sb = reinterpret_cast<const uint8_t*>(s_seq);
  auto base_at = [&](uint32_t s) -> uint32_t { return sb[s + 4u * (s >> 5)] & 3u; };
  uint32_t a = 0;
  // the lane's k-mers once more, for lanes that accepted more than they kept (fn(u, h0) for u = 0 .. n_mine-1)
  auto rehash = [&](auto&& fn) {
    if (single) {
      uint32_t s2 = a + first;
      uint64_t f2 = 0, r2 = 0;
      hash_init(P.hp, [&](uint32_t i) { return base_at(s2 + i); }, f2, r2);
      for (uint32_t u = 0; u < n_mine; ++u) {
        fn(u, f2 + r2);
        const uint32_t cout = base_at(s2), cin = base_at(s2 + k);
        f2 = srol1(f2) ^ s_tab[cin * 4 + cout];
        r2 = sror1(r2 ^ s_tab[16 + cin * 4 + cout]);
        ++s2;
      }
    } else {
      uint64_t j = J0 + first;
      const uint64_t j_end = j + n_mine;
      uint32_t rl = 0, rh = P.n_runs;
      while (rh - rl > 1) {
        const uint32_t mid = rl + ((rh - rl) >> 1);
        if (P.run_vstart[mid] <= j)
          rl = mid;
        else
          rh = mid;
      }
      uint32_t ri = rl;
      while (j < j_end) {
        const uint64_t rv0 = P.run_vstart[ri], rv1 = P.run_vstart[ri + 1];
        const uint64_t seg_end = min(j_end, rv1);
        uint64_t p = P.run_pos[ri] + (j - rv0);
        uint64_t f = 0, r = 0;
        for (uint32_t i = 0; i < k; ++i) {
          f = srol1(f) ^ s_tab[32 + P.code[p + i]];
          r = srol1(r) ^ s_tab[32 + 3 - P.code[p + k - 1 - i]];
        }
        for (;;) {
          fn((uint32_t)(j - J0 - first), f + r);
          ++j;
          if (j >= seg_end) break;
          const uint32_t cout = P.code[p], cin = P.code[p + k];
          f = srol1(f) ^ s_tab[cin * 4 + cout];
          r = sror1(r ^ s_tab[16 + cin * 4 + cout]);
          ++p;
        }
        ++ri;
      }
    }
  };
  if (single) {
    const uint64_t P0 = P.run_pos[lo] + (J0 - v0);
    a = seq_stage(s_seq, P.code, P0, tile_len, k, tid);
    __syncthreads();
    uint32_t s = a + first;
    uint64_t f = 0, r = 0;
    if (n_mine) hash_init(P.hp, [&](uint32_t i) { return base_at(s + i); }, f, r);
#pragma unroll 1
    for (uint32_t b0 = 0; b0 < 32; b0 += 8) {
      uint64_t h[8], idx[8];
      uint32_t sw[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        h[u] = f + r;
        // (hash_roll, nts_tile_sweep.inc, spelled out: through the helper this kernel compiles to other code)
        const uint32_t cout = base_at(s), cin = base_at(s + k);
        f = srol1(f) ^ s_tab[cin * 4 + cout];
        r = sror1(r ^ s_tab[16 + cin * 4 + cout]);
        ++s;
      }
      // three rounds of independent loads (summary, then the filter for the few that passed -- everybody else re-reads word 0,
      // which is cached): a filter read inside the test of each k-mer made eight dependent trips to HBM per batch
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        idx[u] = P.fm(h[u]);
        sw[u] = P.summary[idx[u] >> (P.shift + 5)];
      }
      uint32_t pass = 0, fw[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (b0 + u < n_mine && ((sw[u] >> ((idx[u] >> P.shift) & 31u)) & 1u)) pass |= 1u << u;
#pragma unroll
      for (int u = 0; u < 8; ++u) fw[u] = P.bf[((pass >> u) & 1u) ? (idx[u] >> 5) : 0];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (((pass >> u) & 1u) && ((fw[u] >> ((uint32_t)idx[u] & 31u)) & 1u)) {
          acc_mask |= 1u << (b0 + u);
          if (n_acc < 4) acc_h[n_acc] = h[u];
          ++n_acc;
        }
      }
    }
  } else {
    __syncthreads();
    if (n_mine)
      rehash([&](uint32_t u, uint64_t h) {
        if (accepted(h)) {
          acc_mask |= 1u << u;
          if (n_acc < 4) acc_h[n_acc] = h;
          ++n_acc;
        }
      });
  }
  // the tile's list, in index order: lanes are in index order, a lane's hits too
  uint32_t total = 0;
  const uint32_t before = block_excl_scan_256(n_acc, s_w, &total);
  const uint32_t seg = (uint32_t)(tile % N_SEG);
  if (tid == 0) {
    const unsigned long long base = total ? atomicAdd(&P.seg_count[seg], (unsigned long long)total) : 0ull;
    P.tile_off[tile] = base;
    P.tile_cnt[tile] = total;
    P.tile_ordered[tile] = 1;
    s_base = base;
  }
  __syncthreads();
  if (n_acc == 0 || s_base + total > P.seg_cap) return; // (does not fit: the host sees the counter and retries)
  uint64_t* dj = P.seg_j + (uint64_t)seg * P.seg_cap + s_base + before;
  uint64_t* dk = P.seg_key + (uint64_t)seg * P.seg_cap + s_base + before;
  if (n_acc <= 4) {
    uint32_t q = 0, m = acc_mask;
    while (m) {
      const uint32_t u = (uint32_t)__ffs((int)m) - 1u;
      m &= m - 1;
      dj[q] = J0 + first + u;
      dk[q] = acc_h[q];
      ++q;
    }
  } else {
    uint32_t q = 0;
    rehash([&](uint32_t u, uint64_t h) {
      if ((acc_mask >> u) & 1u) {
        dj[q] = J0 + first + u;
        dk[q] = h;
        ++q;
      }
    });
  }
}

// ---- the same with a first look in LDS ---------------------------------------------------------------------------------------
// k_hash_accept is bound by the L2 -> L1 fills of its summary look-ups (a 128-byte line per 4-byte read: ~10 ms of its 16.7 ms per
// 3 Gbp genome).  When the filter holds few enough set bits, a folded copy of it -- bit (i mod 2^19) = OR of the filter bits
// congruent to i, 64 KiB -- answers about half of the look-ups from LDS: a workgroup of 1024 lanes loads the folded filter once
// and takes four 8192-k-mer tiles (one per 256 lanes, everything else as in k_hash_accept), so that four waves per SIMD share
// one copy.  Only k-mers whose folded bit is set go on to the summary and the filter.
constexpr uint32_t FOLD_BITS_LOG2 = 19;
constexpr uint32_t FOLD_WORDS = (1u << FOLD_BITS_LOG2) / 32; // 16384 words = 64 KiB
constexpr uint32_t ACC4_THREADS = 1024;

struct Accept4Lds
{
  uint32_t fold[FOLD_WORDS];
  uint64_t tab[36];
  uint32_t seq[4][SEQ_LDS_DWORDS];
  uint32_t w[4][8];
  unsigned long long base[4];
};

__global__ __launch_bounds__(ACC4_THREADS) void k_hash_accept4(AcceptParams P, const uint32_t* __restrict__ fold, uint64_t n_tiles)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem4[];
  Accept4Lds& L = *reinterpret_cast<Accept4Lds*>(smem4);
  const uint32_t q = threadIdx.x >> 8, tid = threadIdx.x & 255u;
  {
    const uint4* src = reinterpret_cast<const uint4*>(fold);
    uint4* dst = reinterpret_cast<uint4*>(L.fold);
    for (uint32_t i = threadIdx.x; i < FOLD_WORDS / 4; i += ACC4_THREADS) dst[i] = src[i];
  }
  if (threadIdx.x < 16) {
    L.tab[threadIdx.x] = P.hp.roll_f[threadIdx.x];
    L.tab[16 + threadIdx.x] = P.hp.roll_r[threadIdx.x];
  }
  if (threadIdx.x < 4) L.tab[32 + threadIdx.x] = P.hp.seed[threadIdx.x];
  const uint64_t* s_tab = L.tab;
  uint32_t* s_seq = L.seq[q];
  const uint32_t k = P.hp.k;
  const uint64_t tile = (uint64_t)blockIdx.x * 4 + q;
  const bool have = tile < n_tiles;
  const uint64_t J0 = tile * KEY_TILE;
  const uint32_t tile_len = have ? (uint32_t)min((uint64_t)KEY_TILE, P.n_valid - J0) : 0u;
  uint32_t lo = 0, hi = P.n_runs;
  if (have) {
    while (hi - lo > 1) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (P.run_vstart[mid] <= J0)
        lo = mid;
      else
        hi = mid;
    }
  }
  const uint64_t v0 = have ? P.run_vstart[lo] : 0, v1 = have ? P.run_vstart[lo + 1] : 0;
  const bool single = have && (J0 + tile_len <= v1) && (k <= FAST_K_MAX);
  const uint32_t first = 32u * tid;
  const uint32_t n_mine = first < tile_len ? min(32u, tile_len - first) : 0u;
  uint32_t acc_mask = 0, n_acc = 0;
  uint64_t acc_h[4] = { 0, 0, 0, 0 };
  auto accepted = [&](uint64_t h) -> bool {
    const uint64_t idx = P.fm(h);
    const uint32_t f = (uint32_t)idx & ((1u << FOLD_BITS_LOG2) - 1u);
    if (!((L.fold[f >> 5] >> (f & 31u)) & 1u)) return false;
    const uint64_t g = idx >> P.shift;
    if (!((P.summary[g >> 5] >> (g & 31u)) & 1u)) return false;
    return (P.bf[idx >> 5] >> ((uint32_t)idx & 31u)) & 1u;
  };
  const uint8_t* sb = reinterpret_cast<const uint8_t*>(s_seq);
  auto base_at = [&](uint32_t s) -> uint32_t { return sb[s + 4u * (s >> 5)] & 3u; };
  uint32_t a = 0;
  auto rehash = [&](auto&& fn) {
    if (single) {
      uint32_t s2 = a + first;
      uint64_t f2 = 0, r2 = 0;
      hash_init(P.hp, [&](uint32_t i) { return base_at(s2 + i); }, f2, r2);
      for (uint32_t u = 0; u < n_mine; ++u) {
        fn(u, f2 + r2);
        const uint32_t cout = base_at(s2), cin = base_at(s2 + k);
        f2 = srol1(f2) ^ s_tab[cin * 4 + cout];
        r2 = sror1(r2 ^ s_tab[16 + cin * 4 + cout]);
        ++s2;
      }
    } else {
      uint64_t j = J0 + first;
      const uint64_t j_end = j + n_mine;
      uint32_t rl = 0, rh = P.n_runs;
      while (rh - rl > 1) {
        const uint32_t mid = rl + ((rh - rl) >> 1);
        if (P.run_vstart[mid] <= j)
          rl = mid;
        else
          rh = mid;
      }
      uint32_t ri = rl;
      while (j < j_end) {
        const uint64_t rv0 = P.run_vstart[ri], rv1 = P.run_vstart[ri + 1];
        const uint64_t seg_end = min(j_end, rv1);
        uint64_t p = P.run_pos[ri] + (j - rv0);
        uint64_t f = 0, r = 0;
        for (uint32_t i = 0; i < k; ++i) {
          f = srol1(f) ^ s_tab[32 + P.code[p + i]];
          r = srol1(r) ^ s_tab[32 + 3 - P.code[p + k - 1 - i]];
        }
        for (;;) {
          fn((uint32_t)(j - J0 - first), f + r);
          ++j;
          if (j >= seg_end) break;
          const uint32_t cout = P.code[p], cin = P.code[p + k];
          f = srol1(f) ^ s_tab[cin * 4 + cout];
          r = sror1(r ^ s_tab[16 + cin * 4 + cout]);
          ++p;
        }
        ++ri;
      }
    }
  };
  if (single) {
    const uint64_t P0 = P.run_pos[lo] + (J0 - v0);
    a = seq_stage(s_seq, P.code, P0, tile_len, k, tid);
  }
  __syncthreads(); // folded filter, tables and every quarter's bases are in LDS
  if (single) {
    uint32_t s = a + first;
    uint64_t f = 0, r = 0;
    if (n_mine) hash_init(P.hp, [&](uint32_t i) { return base_at(s + i); }, f, r);
#pragma unroll 1
    for (uint32_t b0 = 0; b0 < 32; b0 += 8) {
      uint64_t h[8], idx[8];
      uint32_t pass = 0;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        h[u] = f + r;
        // (hash_roll, nts_tile_sweep.inc, spelled out: through the helper this kernel compiles to other code)
        const uint32_t cout = base_at(s), cin = base_at(s + k);
        f = srol1(f) ^ s_tab[cin * 4 + cout];
        r = sror1(r ^ s_tab[16 + cin * 4 + cout]);
        ++s;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        idx[u] = P.fm(h[u]);
        const uint32_t fb = (uint32_t)idx[u] & ((1u << FOLD_BITS_LOG2) - 1u);
        if (b0 + u < n_mine && ((L.fold[fb >> 5] >> (fb & 31u)) & 1u)) pass |= 1u << u;
      }
      // about half of the k-mers at config 4's density go on to the L2-resident summary, few of those to the filter; each level
      // as one round of independent loads (lanes that dropped out re-read word 0)
      uint32_t sw[8], fw[8], pass2 = 0;
#pragma unroll
      for (int u = 0; u < 8; ++u) sw[u] = P.summary[((pass >> u) & 1u) ? (idx[u] >> (P.shift + 5)) : 0];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (((pass >> u) & 1u) && ((sw[u] >> ((idx[u] >> P.shift) & 31u)) & 1u)) pass2 |= 1u << u;
#pragma unroll
      for (int u = 0; u < 8; ++u) fw[u] = P.bf[((pass2 >> u) & 1u) ? (idx[u] >> 5) : 0];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (((pass2 >> u) & 1u) && ((fw[u] >> ((uint32_t)idx[u] & 31u)) & 1u)) {
          acc_mask |= 1u << (b0 + u);
          if (n_acc < 4) acc_h[n_acc] = h[u];
          ++n_acc;
        }
      }
    }
  } else if (n_mine) {
    rehash([&](uint32_t u, uint64_t h) {
      if (accepted(h)) {
        acc_mask |= 1u << u;
        if (n_acc < 4) acc_h[n_acc] = h;
        ++n_acc;
      }
    });
  }
  // the quarter's list in index order (exclusive scan over its 256 lanes)
  const uint32_t lane = tid & 63u, wv = tid >> 6;
  uint32_t x = n_acc;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d, 64);
    if (lane >= (uint32_t)d) x += y;
  }
  if (lane == 63) L.w[q][wv] = x;
  __syncthreads();
  uint32_t before = x - n_acc;
  for (uint32_t z = 0; z < wv; ++z) before += L.w[q][z];
  const uint32_t total = L.w[q][0] + L.w[q][1] + L.w[q][2] + L.w[q][3];
  const uint32_t seg = (uint32_t)(tile % N_SEG);
  if (tid == 0 && have) {
    const unsigned long long base = total ? atomicAdd(&P.seg_count[seg], (unsigned long long)total) : 0ull;
    P.tile_off[tile] = base;
    P.tile_cnt[tile] = total;
    P.tile_ordered[tile] = 1;
    L.base[q] = base;
  }
  __syncthreads();
  if (!have || n_acc == 0 || L.base[q] + total > P.seg_cap) return;
  uint64_t* dj = P.seg_j + (uint64_t)seg * P.seg_cap + L.base[q] + before;
  uint64_t* dk = P.seg_key + (uint64_t)seg * P.seg_cap + L.base[q] + before;
  if (n_acc <= 4) {
    uint32_t c = 0, m = acc_mask;
    while (m) {
      const uint32_t u = (uint32_t)__ffs((int)m) - 1u;
      m &= m - 1;
      dj[c] = J0 + first + u;
      dk[c] = acc_h[c];
      ++c;
    }
  } else {
    uint32_t c = 0;
    rehash([&](uint32_t u, uint64_t h) {
      if ((acc_mask >> u) & 1u) {
        dj[c] = J0 + first + u;
        dk[c] = h;
        ++c;
      }
    });
  }
}

// ---- k_hash_accept4r: k_hash_accept4 with the bases in registers -------------------------------------------------------------
// (k <= 32; the host launches k_hash_accept4 otherwise.)  The LDS that held the four tiles' bases is gone; in its place a second
// folded table (128 KiB in all per 1024 lanes: one workgroup per CU).  Of the ~11 ms a 3 Gbp genome took with one table, 6 were
// the lookups behind it -- the summary in the L2 for every second k-mer, the filter in HBM for every 45th (measured with
// NTS_ACC_NO_LOOKUP); two independent tables let about a quarter of the k-mers through instead of half.
struct Accept4rLds
{
  uint32_t fold[2 * FOLD_WORDS]; // bit (index mod 2^19) | bit fold2_slot(index)
  uint64_t tab[36];
  uint32_t w[4][8];
  unsigned long long base[4];
};

// second pass over a lane's k-mers of k_hash_accept4r (a lane not handled from registers, or one with more than four accepted
// k-mers): through the code bytes in global memory, run by run; BODY sees u (index among the lane's k-mers) and h.  (A macro,
// not a lambda taking a lambda: closures that capture the accumulators by reference put them into scratch memory.)
#define ACC4R_REHASH(BODY)                                                                            \
  do {                                                                                                \
    uint64_t j_ = J0 + first;                                                                         \
    const uint64_t j_end_ = j_ + n_mine;                                                              \
    uint32_t rl_ = 0, rh_ = P.n_runs;                                                                 \
    while (rh_ - rl_ > 1) {                                                                           \
      const uint32_t mid_ = rl_ + ((rh_ - rl_) >> 1);                                                 \
      if (P.run_vstart[mid_] <= j_)                                                                   \
        rl_ = mid_;                                                                                   \
      else                                                                                            \
        rh_ = mid_;                                                                                   \
    }                                                                                                 \
    uint32_t ri_ = rl_;                                                                               \
    while (j_ < j_end_) {                                                                             \
      const uint64_t rv0_ = P.run_vstart[ri_], rv1_ = P.run_vstart[ri_ + 1];                          \
      const uint64_t seg_end_ = min(j_end_, rv1_);                                                    \
      uint64_t p_ = P.run_pos[ri_] + (j_ - rv0_);                                                     \
      uint64_t f_ = 0, r_ = 0;                                                                        \
      for (uint32_t i_ = 0; i_ < k; ++i_) {                                                           \
        f_ = srol1(f_) ^ s_tab[32 + P.code[p_ + i_]];                                                 \
        r_ = srol1(r_) ^ s_tab[32 + 3 - P.code[p_ + k - 1 - i_]];                                     \
      }                                                                                               \
      for (;;) {                                                                                      \
        {                                                                                             \
          const uint32_t u = (uint32_t)(j_ - J0 - first);                                             \
          const uint64_t h = f_ + r_;                                                                 \
          BODY                                                                                        \
        }                                                                                             \
        ++j_;                                                                                         \
        if (j_ >= seg_end_) break;                                                                    \
        const uint32_t cout_ = P.code[p_], cin_ = P.code[p_ + k];                                     \
        f_ = srol1(f_) ^ s_tab[cin_ * 4 + cout_];                                                     \
        r_ = sror1(r_ ^ s_tab[16 + cin_ * 4 + cout_]);                                                \
        ++p_;                                                                                         \
      }                                                                                               \
      ++ri_;                                                                                          \
    }                                                                                                 \
  } while (0)

// ACC4R_BLOCK: k-mers hashed, then looked up together (two rounds of independent loads per block)
// FM_FORM: FastMod::mod<FM_FORM> (the form of `h mod bits` fixed at compile time; -1: the run-time field).  With the run-time field
// the compiler kept all three forms and their branches inside the unrolled block of eight k-mers (as in k_bin1).
template <int ACC4R_BLOCK, int FM_FORM>
__global__ __launch_bounds__(ACC4_THREADS) void k_hash_accept4r(AcceptParams P, const uint32_t* __restrict__ pack, const uint32_t* __restrict__ fold, uint64_t n_tiles)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem4r[];
  Accept4rLds& L = *reinterpret_cast<Accept4rLds*>(smem4r);
  const uint32_t q = threadIdx.x >> 8, tid = threadIdx.x & 255u;
  {
    const uint4* src = reinterpret_cast<const uint4*>(fold);
    uint4* dst = reinterpret_cast<uint4*>(L.fold);
    for (uint32_t i = threadIdx.x; i < 2 * FOLD_WORDS / 4; i += ACC4_THREADS) dst[i] = src[i];
  }
  if (threadIdx.x < 16) {
    L.tab[threadIdx.x] = P.hp.roll_f[threadIdx.x];
    L.tab[16 + threadIdx.x] = P.hp.roll_r[threadIdx.x];
  }
  if (threadIdx.x < 4) L.tab[32 + threadIdx.x] = P.hp.seed[threadIdx.x];
  const uint64_t* s_tab = L.tab;
  const uint32_t k = P.hp.k;
  __syncthreads(); // folded filter and tables are in LDS
  // the workgroup keeps its copy of the folded filter and takes one group of four tiles after the other (a workgroup per group
  // spent as long on the copy, the barriers around it and its tail as on its 32 k-mers per lane: one fits a CU at a time)
  for (uint64_t grp = blockIdx.x; grp * 4 < n_tiles; grp += gridDim.x) {
  const uint64_t tile = grp * 4 + q;
  const bool have = tile < n_tiles;
  const uint64_t J0 = tile * KEY_TILE;
  const uint32_t tile_len = have ? (uint32_t)min((uint64_t)KEY_TILE, P.n_valid - J0) : 0u;
  uint32_t lo = 0, hi = P.n_runs;
  if (have) {
    while (hi - lo > 1) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (P.run_vstart[mid] <= J0)
        lo = mid;
      else
        hi = mid;
    }
  }
  const uint64_t v0 = have ? P.run_vstart[lo] : 0, v1 = have ? P.run_vstart[lo + 1] : 0;
  const bool single = have && (J0 + tile_len <= v1) && (k <= FAST_K_MAX);
  const uint32_t first = 32u * tid;
  const uint32_t n_mine = first < tile_len ? min(32u, tile_len - first) : 0u;
  uint32_t acc_mask = 0, n_acc = 0;
  uint64_t acc_h0 = 0, acc_h1 = 0, acc_h2 = 0, acc_h3 = 0; // (named, not an array: indexing one by n_acc put it into scratch memory)
  auto note = [&](uint64_t h) __attribute__((always_inline)) { // (selects of values: stores under an if-chain were merged into one
    acc_h0 = n_acc == 0 ? h : acc_h0;                           //  store through a selected address, which kept all four in memory)
    acc_h1 = n_acc == 1 ? h : acc_h1;
    acc_h2 = n_acc == 2 ? h : acc_h2;
    acc_h3 = n_acc == 3 ? h : acc_h3;
    ++n_acc;
  };
  auto accepted = [&](uint64_t h) __attribute__((always_inline)) -> bool {
    const uint64_t idx = P.fm.template mod<FM_FORM>(h);
    const uint32_t f = (uint32_t)idx & ((1u << FOLD_BITS_LOG2) - 1u);
    if (!((L.fold[f >> 5] >> (f & 31u)) & 1u)) return false;
    const uint32_t f2 = fold2_slot(idx);
    if (!((L.fold[FOLD_WORDS + (f2 >> 5)] >> (f2 & 31u)) & 1u)) return false;
    const uint64_t g = idx >> P.shift;
    if (!((P.summary[g >> 5] >> (g & 31u)) & 1u)) return false;
    return (P.bf[idx >> 5] >> ((uint32_t)idx & 31u)) & 1u;
  };
  // a lane whose 32 k-mers are one stretch of the tile's run takes its outgoing and incoming bases from the 2-bit image of the
  // genome, three words each, in registers (k_hash_select's way: per 16 steps the two streams are woven into 4-bit (incoming,
  // outgoing) pairs, a step forms its roll-table offset with a shift and a mask) -- no staging of the tile's bases in LDS
  const bool regular = single && n_mine == 32u;
  if (regular) {
    const uint64_t xo = P.run_pos[lo] + (J0 - v0) + first;
    const uint32_t sh_o = 2u * ((uint32_t)xo & 15u), sh_i = 2u * ((uint32_t)(xo + k) & 15u);
    const uint32_t* wo = pack + (xo >> 4);
    const uint32_t* wi = pack + ((xo + k) >> 4);
    uint32_t ro[3], ri[3], O[2], I[2];
#pragma unroll
    for (int z = 0; z < 3; ++z) {
      ro[z] = wo[z];
      ri[z] = wi[z];
    }
#pragma unroll
    for (int z = 0; z < 2; ++z) {
      O[z] = __builtin_amdgcn_alignbit(ro[z + 1], ro[z], sh_o);
      I[z] = __builtin_amdgcn_alignbit(ri[z + 1], ri[z], sh_i);
    }
    uint64_t f = 0, r = 0;
    {
      const uint32_t head[4] = { O[0], O[1], 0u, 0u }; // k <= 32: the first k-mer lies in the head of the outgoing stream
      hash_init_packed(P.hp, head, f, r);
    }
    const uint8_t* const tab_bytes = reinterpret_cast<const uint8_t*>(s_tab);
#pragma unroll
    for (int z = 0; z < 2; ++z) {
      const uint32_t even = (O[z] & 0x33333333u) | ((I[z] & 0x33333333u) << 2);
      const uint32_t odd = ((O[z] >> 2) & 0x33333333u) | (I[z] & 0xCCCCCCCCu);
#pragma unroll
      for (int b8 = 0; b8 < 16; b8 += ACC4R_BLOCK) {
        const uint32_t b0 = 16u * z + b8;
        uint64_t h[ACC4R_BLOCK], idx[ACC4R_BLOCK];
        uint32_t pass = 0;
#pragma unroll
        for (int u = 0; u < ACC4R_BLOCK; ++u) {
          const int j = b8 + u;
          const uint32_t pairs = (j & 1) ? odd : even;
          const int sh = 4 * (j >> 1) - 3;
          const uint32_t t8 = (sh < 0 ? pairs << 3 : pairs >> sh) & 0x78u; // 8 * (4 * incoming + outgoing)
          h[u] = f + r;
          f = srol1(f) ^ *reinterpret_cast<const uint64_t*>(tab_bytes + t8);
          r = sror1(r ^ *reinterpret_cast<const uint64_t*>(tab_bytes + 128 + t8));
        }
#pragma unroll
        for (int u = 0; u < ACC4R_BLOCK; ++u) {
          idx[u] = P.fm.template mod<FM_FORM>(h[u]);
          const uint32_t fb = (uint32_t)idx[u] & ((1u << FOLD_BITS_LOG2) - 1u);
          const uint32_t f2 = fold2_slot(idx[u]);
          if (((L.fold[fb >> 5] >> (fb & 31u)) & (L.fold[FOLD_WORDS + (f2 >> 5)] >> (f2 & 31u))) & 1u) pass |= 1u << u;
        }
        pass &= P.probe_mask;
        uint32_t sw[ACC4R_BLOCK], fw[ACC4R_BLOCK], pass2 = 0;
#pragma unroll
        for (int u = 0; u < ACC4R_BLOCK; ++u) sw[u] = P.summary[((pass >> u) & 1u) ? (idx[u] >> (P.shift + 5)) : 0];
#pragma unroll
        for (int u = 0; u < ACC4R_BLOCK; ++u)
          if (((pass >> u) & 1u) && ((sw[u] >> ((idx[u] >> P.shift) & 31u)) & 1u)) pass2 |= 1u << u;
#pragma unroll
        for (int u = 0; u < ACC4R_BLOCK; ++u) fw[u] = P.bf[((pass2 >> u) & 1u) ? (idx[u] >> 5) : 0];
#pragma unroll
        for (int u = 0; u < ACC4R_BLOCK; ++u) {
          if (((pass2 >> u) & 1u) && ((fw[u] >> ((uint32_t)idx[u] & 31u)) & 1u)) {
            acc_mask |= 1u << (b0 + u);
            note(h[u]);
          }
        }
      }
    }
  } else if (n_mine) {
    ACC4R_REHASH(if (accepted(h)) {
      acc_mask |= 1u << u;
      note(h);
    });
  }
  // the quarter's list in index order (exclusive scan over its 256 lanes)
  const uint32_t lane = tid & 63u, wv = tid >> 6;
  uint32_t x = n_acc;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d, 64);
    if (lane >= (uint32_t)d) x += y;
  }
  if (lane == 63) L.w[q][wv] = x;
  __syncthreads();
  uint32_t before = x - n_acc;
  for (uint32_t z = 0; z < wv; ++z) before += L.w[q][z];
  const uint32_t total = L.w[q][0] + L.w[q][1] + L.w[q][2] + L.w[q][3];
  const uint32_t seg = (uint32_t)(tile % N_SEG);
  if (tid == 0 && have) {
    const unsigned long long base = total ? atomicAdd(&P.seg_count[seg], (unsigned long long)total) : 0ull;
    P.tile_off[tile] = base;
    P.tile_cnt[tile] = total;
    P.tile_ordered[tile] = 1;
    L.base[q] = base;
  }
  __syncthreads();
  if (!have || n_acc == 0 || L.base[q] + total > P.seg_cap) continue;
  uint64_t* dj = P.seg_j + (uint64_t)seg * P.seg_cap + L.base[q] + before;
  uint64_t* dk = P.seg_key + (uint64_t)seg * P.seg_cap + L.base[q] + before;
  if (n_acc <= 4) {
    uint32_t c = 0, m = acc_mask;
    while (m) {
      const uint32_t u = (uint32_t)__ffs((int)m) - 1u;
      m &= m - 1;
      dj[c] = J0 + first + u;
      dk[c] = c == 0 ? acc_h0 : c == 1 ? acc_h1 : c == 2 ? acc_h2 : acc_h3;
      ++c;
    }
  } else {
    uint32_t c = 0;
    ACC4R_REHASH(if ((acc_mask >> u) & 1u) {
      dj[c] = J0 + first + u;
      dk[c] = h;
      ++c;
    });
  }
  } // groups of four tiles
}
#undef ACC4R_REHASH

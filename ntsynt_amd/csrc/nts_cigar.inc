// ---- one CIGAR per chain of aligned pieces (nts_cigar_build; ntsynt_amd/assess.py block_alignments) ----
// docs/design/04_22_block_alignments.md.  Input: n_pieces pieces {chain, n, m, flags} in chain order, the ops of all pieces one behind
// the other (what the three script calls deliver, seg = the piece's index, p and q local to the piece) and first[n_pieces + 1].  A piece
// with D ops owns 2 D + 1 ATOMS: match run, op, match run, ..., trailing match run; piece t's atoms lie at slots 2 first[t] + t ..
// 2 first[t + 1] + t, mirrored for a reversed piece.  An atom is {len << 4 | code, chain}: the encoding of a CIGAR entry.
//   1  k_cig_atoms: one lane per op and one per piece (the trailing run).  A lane reads the previous op of its piece, checks the column
//      rules and stores its atoms; a lane whose ops break a rule stores empty atoms and its piece's index in the status array.  A
//      minimum reduction of the status array names the smallest offending piece (timer "cigar_atoms").
//   2  rocprim::select drops the atoms of length 0; the host reads the status and the number M of atoms that are left.
//   3  rocprim::reduce_by_key over (chain, code) adds the lengths of every maximal run of one kind inside one chain: the entries;
//      k_cig_emit packs them.  A second rocprim::reduce_by_key over the chain adds up, per chain, the heads (atoms whose (chain, code)
//      differs from their predecessor's) and the columns of each kind; k_cig_chain_sums stores the sums at their chain, an exclusive
//      scan of the entry counts over ALL chains gives `first`, k_cig_chains writes the records (timer "cigar_merge").
// No genome is read.  No atomic, no launch per piece or chain, no floating point, no host loop beyond the O(n_pieces) checks.

constexpr uint64_t CIG_I = 1, CIG_D = 2, CIG_EQ = 7, CIG_X = 8; // BAM's codes
constexpr uint64_t CIG_P = 6;                                   // BAM's padding: what nts_cigar_pad adds and nts_cigar_rows_padded alone reads
constexpr uint64_t CIG_MAX_COLUMNS = 1ull << 60;               // len << 4 stays inside 64 bits

// the last i < n whose key(i) <= e over nondecreasing keys, 0 where there is none (n >= 1): the piece of an op, the chain of an
// entry, the entry of a text byte
template <class I, class Key>
__device__ __forceinline__ I cig_last_at_or_before(I n, uint64_t e, Key key)
{
  I lo = 0, hi = n;
  while (hi - lo > 1u) {
    const I mid = lo + (hi - lo) / 2u;
    if (key(mid) <= e) lo = mid;
    else hi = mid;
  }
  return lo;
}

struct CigAtom
{
  uint64_t run; // len << 4 | code
  uint32_t chain, pad;
};
static_assert(sizeof(CigAtom) == 16, "one atom, one 16-byte store");
static_assert(sizeof(nts_cig_piece) == 16 && sizeof(nts_cig_chain) == 64, "the C ABI's layout");

struct CigSums // what one atom adds to its chain, and the sum of those
{
  uint64_t n_cig, eq, x, ins, del;
};

struct CigHasLength
{
  __host__ __device__ bool operator()(const CigAtom& a) const { return (a.run >> 4) != 0; }
};

struct CigKeyOf // runs merge where chain and code are equal
{
  __host__ __device__ uint64_t operator()(const CigAtom& a) const { return (uint64_t)a.chain << 4 | (a.run & 15u); }
};

struct CigLenOf
{
  __host__ __device__ uint64_t operator()(const CigAtom& a) const { return a.run >> 4; }
};

struct CigChainOf
{
  __host__ __device__ uint32_t operator()(const CigAtom& a) const { return a.chain; }
};

struct CigAtomSums // kept atom i: a head opens an entry; its columns by kind
{
  const CigAtom* atoms;
  __host__ __device__ CigSums operator()(uint32_t i) const
  {
    const CigAtom a = atoms[i];
    const uint64_t code = a.run & 15u, len = a.run >> 4;
    bool head = i == 0;
    if (!head) {
      const CigAtom b = atoms[i - 1];
      head = b.chain != a.chain || (b.run & 15u) != code;
    }
    return { head ? 1ull : 0ull, code == CIG_EQ ? len : 0, code == CIG_X ? len : 0, code == CIG_I ? len : 0, code == CIG_D ? len : 0 };
  }
};

struct CigSumsAdd
{
  __host__ __device__ CigSums operator()(const CigSums& a, const CigSums& b) const
  {
    return { a.n_cig + b.n_cig, a.eq + b.eq, a.x + b.x, a.ins + b.ins, a.del + b.del };
  }
};

struct CigEntriesOf
{
  __host__ __device__ uint64_t operator()(const CigSums& s) const { return s.n_cig; }
};

__global__ __launch_bounds__(256) void k_cig_atoms(const nts_cig_piece* __restrict__ pieces, uint32_t n_pieces, const nts_edit_op* __restrict__ ops,
                                                   uint32_t n_ops, const uint64_t* __restrict__ first, CigAtom* __restrict__ atoms, uint64_t n_atoms,
                                                   uint32_t* __restrict__ status)
{
  const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x; // lanes 0 .. n_ops - 1: an op each; then a piece each
  if (g >= (uint64_t)n_ops + n_pieces) return;
  const bool trailing = g >= n_ops;
  uint32_t t;
  bool ok = true;
  if (trailing) {
    t = (uint32_t)(g - n_ops);
  } else {
    t = ops[g].seg;
    if (t >= n_pieces || g < first[t] || g >= first[t + 1]) { // seg is not the piece that owns op g: find that piece, the last with first[t] <= g
      t = cig_last_at_or_before(n_pieces, g, [first](uint32_t i) { return first[i]; }); // (first[0] = 0 <= g < n_ops = first[n_pieces])
      ok = false;
    }
  }
  const nts_cig_piece pc = pieces[t];
  const uint64_t f0 = first[t], f1 = first[t + 1];
  // (the host refused this before the launch: a lane still touches nothing outside the ops and its piece's atoms)
  if (f1 < f0 || f1 > n_ops || (!trailing && (g < f0 || g >= f1))) {
    status[g] = t;
    return;
  }
  const uint64_t D = f1 - f0, j = trailing ? D : g - f0; // this lane: the match run in front of op j and op j, or the run behind the last op
  uint64_t i0 = 0, j0 = 0;                               // where the piece stands behind op j - 1
  if (j > 0) {
    const nts_edit_op pv = ops[f0 + j - 1]; // (f0 <= f0 + j - 1 < f1 <= n_ops)
    i0 = (uint64_t)pv.p + (pv.op != NTS_OP_INS ? 1u : 0u);
    j0 = (uint64_t)pv.q + (pv.op != NTS_OP_DEL ? 1u : 0u);
  }
  const uint64_t n = pc.n, m = pc.m;
  uint64_t run = 0, code = 0;
  if (trailing) {
    ok = ok && i0 <= n && j0 <= m && n - i0 == m - j0;
    run = n - i0;
  } else {
    const nts_edit_op op = ops[g];
    const uint64_t p = op.p, q = op.q;
    ok = ok && p >= i0 && q >= j0 && p - i0 == q - j0;
    if (op.op == NTS_OP_SUB) ok = ok && p < n && q < m, code = CIG_X;
    else if (op.op == NTS_OP_DEL) ok = ok && p < n && q <= m, code = CIG_D;
    else if (op.op == NTS_OP_INS) ok = ok && p <= n && q < m, code = CIG_I;
    else ok = false;
    run = p - i0;
  }
  if (!ok) run = 0; // (empty atoms: the selection drops them; the call returns no CIGAR anyway)
  const uint64_t base = 2u * f0 + t, last = 2u * D;      // the piece's atoms: slots base .. base + 2 D
  const bool mirrored = (pc.flags & NTS_CIG_REVERSED) != 0;
  const uint64_t at_run = base + (mirrored ? last - 2u * j : 2u * j);
  if (at_run < n_atoms) atoms[at_run] = { run << 4 | CIG_EQ, pc.chain, 0u };
  if (!trailing) {
    const uint64_t at_op = base + (mirrored ? last - 2u * j - 1u : 2u * j + 1u); // (j < D: 2 j + 1 <= 2 D - 1)
    if (at_op < n_atoms) atoms[at_op] = { (ok ? 1ull << 4 : 0ull) | code, pc.chain, 0u };
  }
  status[g] = ok ? SCRIPT_OK : t;
}

// entry e = the summed length and the code of run e
__global__ __launch_bounds__(256) void k_cig_emit(const uint64_t* __restrict__ key, const uint64_t* __restrict__ len, const uint64_t* __restrict__ n_entries,
                                                  uint64_t cap, uint64_t* __restrict__ out)
{
  const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (e >= cap || e >= *n_entries) return;
  out[e] = len[e] << 4 | (key[e] & 15u);
}

// the sums of the chains that have an atom, each at its chain (every other chain keeps its zeros)
__global__ __launch_bounds__(256) void k_cig_chain_sums(const uint32_t* __restrict__ chain, const CigSums* __restrict__ sums, const uint64_t* __restrict__ n_keys,
                                                        uint64_t cap, uint64_t n_chains, CigSums* __restrict__ out)
{
  const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (j >= cap || j >= *n_keys) return;
  const uint32_t c = chain[j];
  if (c < n_chains) out[c] = sums[j];
}

__global__ __launch_bounds__(256) void k_cig_chains(const CigSums* __restrict__ sums, const uint64_t* __restrict__ first, uint64_t n_chains,
                                                    nts_cig_chain* __restrict__ out)
{
  const uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (c >= n_chains) return;
  const CigSums s = sums[c];
  out[c] = { first[c], s.n_cig, s.eq, s.x, s.ins, s.del, s.eq + s.x + s.del, s.eq + s.x + s.ins };
}

int cigar_build_run(nts_ctx* ctx, const nts_cig_piece* pieces, uint64_t n_pieces, uint64_t n_chains, const nts_edit_op* ops, const uint64_t* first,
                    uint64_t** cigar, uint64_t* n_cigar, nts_cig_chain* chains)
{
  if (n_pieces > 0xFFFFFFFFull || n_chains > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_cigar_build: 2^32 pieces or chains or more");
  if (first[0] != 0) return fail(ctx, NTS_EINVAL, "nts_cigar_build: first does not start at 0 (piece 0)");
  uint64_t columns = 0;
  for (uint64_t t = 0; t < n_pieces; ++t) {
    const nts_cig_piece& pc = pieces[t];
    auto who = [t] { return "nts_cigar_build: piece " + std::to_string(t); }; // (made only for a piece that is refused)
    if (pc.chain >= n_chains) return fail(ctx, NTS_EINVAL, who() + " names a chain at or beyond n_chains");
    if (t && pc.chain < pieces[t - 1].chain) return fail(ctx, NTS_EINVAL, who() + ": the pieces are not in chain order");
    if (pc.flags & ~NTS_CIG_REVERSED) return fail(ctx, NTS_EINVAL, who() + " has unknown flag bits");
    if (first[t + 1] < first[t]) return fail(ctx, NTS_EINVAL, who() + ": first is not nondecreasing");
    columns += (uint64_t)pc.n + pc.m;
    if (columns >= CIG_MAX_COLUMNS) return fail(ctx, NTS_ERANGE, "nts_cigar_build: 2^60 bases or more");
  }
  const uint64_t n_ops = first[n_pieces];
  if (n_ops > 0xFFFFFFFFull || 2 * n_ops + n_pieces > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_cigar_build: 2^32 atoms or more (2 ops + pieces)");
  if (n_ops && !ops) return fail(ctx, NTS_EINVAL, "nts_cigar_build: bad arguments (no ops)");
  *cigar = nullptr;
  *n_cigar = 0;
  if (n_pieces == 0) { // (nothing is launched)
    if (n_chains) memset(chains, 0, n_chains * sizeof(nts_cig_chain));
    return NTS_OK;
  }
  const uint64_t n_atoms = 2 * n_ops + n_pieces, lanes = n_ops + n_pieces;
  NTS_WS(d_pieces, nts_cig_piece*, "cig_pieces", n_pieces * sizeof(nts_cig_piece));
  NTS_WS(d_ops, nts_edit_op*, "cig_ops", std::max<uint64_t>(n_ops, 1) * sizeof(nts_edit_op));
  NTS_WS(d_first, uint64_t*, "cig_first", (n_pieces + 1) * 8);
  NTS_WS(d_atoms, CigAtom*, "cig_atoms", n_atoms * sizeof(CigAtom));
  NTS_WS(d_kept, CigAtom*, "cig_kept", n_atoms * sizeof(CigAtom));
  NTS_WS(d_status, uint32_t*, "cig_status", lanes * 4);
  NTS_WS(d_num, uint64_t*, "cig_num", 4 * 8); // worst (as uint32), kept atoms, entries, chains with an atom
  uint32_t* const d_worst = (uint32_t*)d_num;
  hipError_t e_run = hipMemcpyAsync(d_pieces, pieces, n_pieces * sizeof(nts_cig_piece), hipMemcpyHostToDevice, ctx->stream);
  if (e_run == hipSuccess && n_ops) e_run = hipMemcpyAsync(d_ops, ops, n_ops * sizeof(nts_edit_op), hipMemcpyHostToDevice, ctx->stream);
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(d_first, first, (n_pieces + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
  uint32_t worst = SCRIPT_OK;
  uint64_t kept = 0;
  if (e_run == hipSuccess) {
    ScopedTimer t(ctx, "cigar_atoms", true);
    NTS_LAUNCH(k_cig_atoms, IVL_GRID(lanes), (const nts_cig_piece*)d_pieces, (uint32_t)n_pieces, (const nts_edit_op*)d_ops, (uint32_t)n_ops,
               (const uint64_t*)d_first, d_atoms, n_atoms, d_status);
    size_t tmp = 0;
    e_run = rocprim::reduce(nullptr, tmp, d_status, d_worst, SCRIPT_OK, lanes, ScriptMin(), ctx->stream);
    void* d_tmp = e_run == hipSuccess ? ws_get(ctx, "ivs_tmp", std::max<size_t>(tmp, 16)) : nullptr;
    if (e_run == hipSuccess && !d_tmp) e_run = hipErrorOutOfMemory;
    if (e_run == hipSuccess) e_run = rocprim::reduce(d_tmp, tmp, d_status, d_worst, SCRIPT_OK, lanes, ScriptMin(), ctx->stream);
  }
  if (e_run == hipSuccess) {
    ScopedTimer t(ctx, "cigar_merge");
    size_t tmp = 0;
    e_run = rocprim::select(nullptr, tmp, d_atoms, d_kept, d_num + 1, n_atoms, CigHasLength(), ctx->stream);
    void* d_tmp = e_run == hipSuccess ? ws_get(ctx, "ivs_tmp", std::max<size_t>(tmp, 16)) : nullptr;
    if (e_run == hipSuccess && !d_tmp) e_run = hipErrorOutOfMemory;
    if (e_run == hipSuccess) e_run = rocprim::select(d_tmp, tmp, d_atoms, d_kept, d_num + 1, n_atoms, CigHasLength(), ctx->stream);
  }
  if (e_run == hipSuccess) e_run = hipGetLastError();
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(&worst, d_worst, 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(&kept, d_num + 1, 8, hipMemcpyDeviceToHost, ctx->stream);
  hipError_t e_sync = hipStreamSynchronize(ctx->stream); // (whatever happened: the caller's arrays were sources of asynchronous copies)
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  if (worst != SCRIPT_OK) return fail(ctx, NTS_EINVAL, "nts_cigar_build: ops of piece " + std::to_string(worst) + " are no script of its lengths");
  if (kept > n_atoms) return fail(ctx, NTS_EHIP, "nts_cigar_build: the selection kept more atoms than there are");
  if (kept == 0) { // (every piece is empty: no entry, every record 0)
    if (n_chains) memset(chains, 0, n_chains * sizeof(nts_cig_chain));
    return NTS_OK;
  }
  NTS_WS(d_ekey, uint64_t*, "cig_ekey", kept * 8);
  NTS_WS(d_elen, uint64_t*, "cig_elen", kept * 8);
  NTS_WS(d_entries, uint64_t*, "cig_entries", kept * 8);
  NTS_WS(d_asums, CigSums*, "cig_asums", kept * sizeof(CigSums));
  NTS_WS(d_uchain, uint32_t*, "cig_uchain", kept * 4);
  NTS_WS(d_csums, CigSums*, "cig_csums", n_chains * sizeof(CigSums));
  NTS_WS(d_cfirst, uint64_t*, "cig_cfirst", n_chains * 8);
  NTS_WS(d_chains, nts_cig_chain*, "cig_chains", n_chains * sizeof(nts_cig_chain));
  uint64_t n_entries = 0;
  {
    ScopedTimer t(ctx, "cigar_merge");
    auto keys = rocprim::make_transform_iterator((const CigAtom*)d_kept, CigKeyOf());
    auto lens = rocprim::make_transform_iterator((const CigAtom*)d_kept, CigLenOf());
    auto chain_of = rocprim::make_transform_iterator((const CigAtom*)d_kept, CigChainOf());
    auto sums_of = rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0), CigAtomSums{ d_kept });
    auto entries_of = rocprim::make_transform_iterator((const CigSums*)d_csums, CigEntriesOf());
    size_t tmp_e = 0, tmp_c = 0, tmp_f = 0;
    e_run = rocprim::reduce_by_key(nullptr, tmp_e, keys, lens, kept, d_ekey, d_elen, d_num + 2, rocprim::plus<uint64_t>(), rocprim::equal_to<uint64_t>(),
                                   ctx->stream);
    if (e_run == hipSuccess)
      e_run = rocprim::reduce_by_key(nullptr, tmp_c, chain_of, sums_of, kept, d_uchain, d_asums, d_num + 3, CigSumsAdd(), rocprim::equal_to<uint32_t>(),
                                     ctx->stream);
    if (e_run == hipSuccess)
      e_run = rocprim::exclusive_scan(nullptr, tmp_f, entries_of, d_cfirst, (uint64_t)0, n_chains, rocprim::plus<uint64_t>(), ctx->stream);
    void* d_tmp = e_run == hipSuccess ? ws_get(ctx, "ivs_tmp", std::max<size_t>(std::max(tmp_e, std::max(tmp_c, tmp_f)), 16)) : nullptr;
    if (e_run == hipSuccess && !d_tmp) e_run = hipErrorOutOfMemory;
    if (e_run == hipSuccess)
      e_run = rocprim::reduce_by_key(d_tmp, tmp_e, keys, lens, kept, d_ekey, d_elen, d_num + 2, rocprim::plus<uint64_t>(), rocprim::equal_to<uint64_t>(),
                                     ctx->stream);
    if (e_run == hipSuccess)
      NTS_LAUNCH(k_cig_emit, IVL_GRID(kept), (const uint64_t*)d_ekey, (const uint64_t*)d_elen, (const uint64_t*)(d_num + 2), kept, d_entries);
    if (e_run == hipSuccess)
      e_run = rocprim::reduce_by_key(d_tmp, tmp_c, chain_of, sums_of, kept, d_uchain, d_asums, d_num + 3, CigSumsAdd(), rocprim::equal_to<uint32_t>(),
                                     ctx->stream);
    if (e_run == hipSuccess) e_run = hipMemsetAsync(d_csums, 0, n_chains * sizeof(CigSums), ctx->stream);
    if (e_run == hipSuccess) {
      NTS_LAUNCH(k_cig_chain_sums, IVL_GRID(kept), (const uint32_t*)d_uchain, (const CigSums*)d_asums, (const uint64_t*)(d_num + 3), kept, n_chains, d_csums);
      e_run = rocprim::exclusive_scan(d_tmp, tmp_f, entries_of, d_cfirst, (uint64_t)0, n_chains, rocprim::plus<uint64_t>(), ctx->stream);
    }
    if (e_run == hipSuccess) NTS_LAUNCH(k_cig_chains, IVL_GRID(n_chains), (const CigSums*)d_csums, (const uint64_t*)d_cfirst, n_chains, d_chains);
  }
  if (e_run == hipSuccess) e_run = hipGetLastError();
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(&n_entries, d_num + 2, 8, hipMemcpyDeviceToHost, ctx->stream);
  e_sync = hipStreamSynchronize(ctx->stream);
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  if (n_entries == 0 || n_entries > kept) return fail(ctx, NTS_EHIP, "nts_cigar_build: the merge left an impossible number of entries");
  uint64_t* host_cigar = (uint64_t*)malloc(n_entries * 8);
  nts_cig_chain* host_chains = (nts_cig_chain*)malloc(n_chains * sizeof(nts_cig_chain)); // (the caller's array is written only when the call succeeds)
  if (!host_cigar || !host_chains) {
    free(host_cigar);
    free(host_chains);
    return fail(ctx, NTS_ENOMEM, "nts_cigar_build: no host memory for the CIGAR");
  }
  e_run = hipMemcpyAsync(host_cigar, d_entries, n_entries * 8, hipMemcpyDeviceToHost, ctx->stream);
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(host_chains, d_chains, n_chains * sizeof(nts_cig_chain), hipMemcpyDeviceToHost, ctx->stream);
  e_sync = hipStreamSynchronize(ctx->stream);
  if (e_run == hipSuccess && e_sync == hipSuccess) memcpy(chains, host_chains, n_chains * sizeof(nts_cig_chain));
  else free(host_cigar);
  free(host_chains);
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  *cigar = host_cigar;
  *n_cigar = n_entries;
  return NTS_OK;
}

// ---- the staged prefix index of a round's CIGARs: what nts_cigar_lift, nts_cigar_lift_stats and nts_cigar_text share ----
// Each of the three reads CIGAR entries and chain records as nts_cigar_build returns them, and each begins alike: cig_chains_check
// looks at the records on the host; cig_index_stage copies entries and records to the device (the context's "cigx_*" buffers: one
// name set, so a run of all three keeps one copy), runs ONE rocprim::exclusive_scan over n_cigar + 1 elements of what the caller's
// transform functor makes of an entry -- a tuple whose first two members are the (A bases, B bases) it consumes, zeros for the element
// behind the last -- into NP columns of n_cigar + 1 GLOBAL prefixes, the last row holding the totals (a chain-local prefix is
// P[e] - P[first]), and then k_lift_check: one lane per entry (a code outside {1, 2, 7, 8}, a length of 0, a prefix that wrapped) and
// one per chain (P[first + n_cig] - P[first] is not its len_a / len_b); a flagged lane stores its chain's index in its status word, a
// minimum reduction names the smallest.  All of it runs under the caller's timer name.

using CigBases = rocprim::tuple<uint64_t, uint64_t>; // (A bases, B bases)

// what an entry consumes on either side
__host__ __device__ inline CigBases cig_bases(uint64_t v)
{
  const uint64_t code = v & 15u, len = v >> 4;
  const bool both = code == CIG_EQ || code == CIG_X;
  return CigBases(both || code == CIG_D ? len : 0, both || code == CIG_I ? len : 0);
}

struct CigTupleAdd // member by member, for a tuple of any arity
{
  template <class T, size_t... K>
  static __host__ __device__ T add(const T& x, const T& y, std::index_sequence<K...>)
  {
    return T((rocprim::get<K>(x) + rocprim::get<K>(y))...);
  }
  template <class... U>
  __host__ __device__ rocprim::tuple<U...> operator()(const rocprim::tuple<U...>& x, const rocprim::tuple<U...>& y) const
  {
    return add(x, y, std::index_sequence_for<U...>());
  }
};

// the entry of base `pos` of one side of a chain with entries [lo, hi) over that side's prefix P, base = P[chain's first]: the
// smallest hi with P[lo] - base <= pos < P[hi] - base narrows to lo + 1 (k_lift_check: P[first + n_cig] - base is the side's length)
__device__ __forceinline__ uint64_t cig_entry_of(const uint64_t* __restrict__ P, uint64_t base, uint64_t lo, uint64_t hi, uint64_t pos)
{
  while (hi - lo > 1u) {
    const uint64_t mid = lo + (hi - lo) / 2u;
    if (P[mid] - base > pos) hi = mid;
    else lo = mid;
  }
  return lo;
}

// the record of a query's or range's {chain, side}: false, and nothing read, for a chain or a side that is none
__device__ __forceinline__ bool cig_chain_of(const nts_cig_chain* __restrict__ chains, uint64_t n_chains, uint32_t chain, uint32_t side, nts_cig_chain& ch)
{
  if (chain >= n_chains || side > 1u) return false;
  ch = chains[chain];
  return true;
}

// a record whose entries reach beyond n_cigar (the host refused it before the launch: a lane still reads nothing outside the prefixes)
__device__ __forceinline__ bool cig_chain_beyond(const nts_cig_chain& ch, uint64_t n_cigar) { return ch.first > n_cigar || ch.n_cig > n_cigar - ch.first; }

// PADDED: an entry of code 6 (P, padding: a column that consumes nothing) passes as well -- for nts_cigar_rows_padded alone
template <bool PADDED>
__global__ __launch_bounds__(256) void k_lift_check(const uint64_t* __restrict__ cigar, uint64_t n_cigar, const nts_cig_chain* __restrict__ chains,
                                                    uint64_t n_chains, const uint64_t* __restrict__ PA, const uint64_t* __restrict__ PB,
                                                    uint32_t* __restrict__ status)
{
  const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x; // lanes 0 .. n_cigar - 1: an entry each; then a chain each
  if (g >= n_cigar + n_chains) return;
  uint32_t say = SCRIPT_OK;
  if (g < n_cigar) {
    const uint64_t v = cigar[g], code = v & 15u;
    const bool bad = (code != CIG_I && code != CIG_D && code != CIG_EQ && code != CIG_X && !(PADDED && code == CIG_P)) || (v >> 4) == 0 ||
                     PA[g + 1] < PA[g] || PB[g + 1] < PB[g];
    // its chain: the last whose first <= g, chain 0 for an entry in front of every chain (on this error path only)
    if (bad && n_chains) say = (uint32_t)cig_last_at_or_before(n_chains, g, [chains](uint64_t c) { return chains[c].first; });
  } else {
    const uint64_t c = g - n_cigar;
    const nts_cig_chain ch = chains[c];
    if (cig_chain_beyond(ch, n_cigar) || PA[ch.first + ch.n_cig] - PA[ch.first] != ch.len_a ||
        PB[ch.first + ch.n_cig] - PB[ch.first] != ch.len_b)
      say = (uint32_t)c;
  }
  status[g] = say;
}

// The chain records, on the host, for entry point `name`: `first` nondecreasing and first + n_cig inside the entries -- with `tile`,
// the chains one behind the other over all entries instead -- and fewer than 2^limit_log2 bases a side over all chains: the global
// scan, and what the caller adds up beside it, must not wrap.  per_chain(c, who) -> a return code: the caller's own checks of chain c,
// behind these; who() makes "name: chain c" (only for a chain that is refused).
template <class PerChain>
int cig_chains_check(nts_ctx* ctx, const char* name, uint32_t limit_log2, bool tile, const nts_cig_chain* chains, uint64_t n_chains, uint64_t n_cigar,
                     PerChain per_chain)
{
  const uint64_t limit = 1ull << limit_log2;
  auto too_many = [&] { return fail(ctx, NTS_ERANGE, std::string(name) + ": 2^" + std::to_string(limit_log2) + " bases or more"); };
  uint64_t next = 0, sum_a = 0, sum_b = 0;
  for (uint64_t c = 0; c < n_chains; ++c) {
    const nts_cig_chain& ch = chains[c];
    auto who = [name, c] { return std::string(name) + ": chain " + std::to_string(c); };
    if (tile) {
      if (ch.first != next || ch.n_cig > n_cigar - next) return fail(ctx, NTS_EINVAL, who() + ": the chains do not tile the entries");
      next += ch.n_cig;
    } else {
      if (c && ch.first < chains[c - 1].first) return fail(ctx, NTS_EINVAL, who() + ": first is not nondecreasing");
      if (ch.first > n_cigar || ch.n_cig > n_cigar - ch.first) return fail(ctx, NTS_EINVAL, who() + ": first + n_cig lies beyond n_cigar");
    }
    if (ch.len_a >= limit || ch.len_b >= limit) return too_many();
    sum_a += ch.len_a;
    sum_b += ch.len_b;
    if (sum_a >= limit || sum_b >= limit) return too_many();
    if (const int rc = per_chain(c, who)) return rc;
  }
  if (tile && next != n_cigar)
    return fail(ctx, NTS_EINVAL, n_chains ? std::string(name) + ": chain " + std::to_string(n_chains - 1) + ": the chains do not tile the entries (the last one ends in front of n_cigar)"
                                          : std::string(name) + ": entries and no chain: the chains do not tile the entries");
  return NTS_OK;
}

struct CigIndex // what cig_index_stage leaves in the context's workspace: dead behind the next call of any of the three readers
{
  const uint64_t* cigar;       // "cigx_cigar": the entries
  const nts_cig_chain* chains; // "cigx_chains": the records
  uint64_t* prefixes;          // "cigx_prefixes": NP columns of `rows` = n_cigar + 1 words; 0: A bases, 1: B bases, then the caller's own
  uint64_t rows;
  uint32_t* status;            // "cigx_status": max(n_cigar + n_chains, n_items) words; the caller's lanes write it behind k_lift_check's
  uint32_t* worst;             // "cigx_worst": [0] the smallest offending chain, [1] for the caller's reduction
  void* tmp;                   // "ivs_tmp", large enough for a ScriptMin reduction of that many status words: tmp_bytes
  size_t tmp_bytes;
  const uint64_t* column(uint32_t k) const { return prefixes + k * rows; }
};

// whether a scan functor reads padded entries: one that says `static constexpr bool PADDED = true` (CigRowsOf<true>); no other does
template <class Of, class = void>
struct CigOfPadded
{
  static constexpr bool value = false;
};
template <class Of>
struct CigOfPadded<Of, std::enable_if_t<Of::PADDED>>
{
  static constexpr bool value = true;
};

// the scan of Of's tuples into the columns (the size query with tmp = nullptr)
template <class Of, size_t... K>
hipError_t cig_index_scan(void* tmp, size_t& bytes, const CigIndex& ix, uint64_t n_cigar, hipStream_t stream, std::index_sequence<K...>)
{
  auto adds = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), Of{ ix.cigar, n_cigar });
  auto prefixes = rocprim::make_zip_iterator(rocprim::make_tuple((ix.prefixes + K * ix.rows)...));
  return rocprim::exclusive_scan(tmp, bytes, adds, prefixes, typename Of::Tuple((uint64_t)(0 * K)...), n_cigar + 1, CigTupleAdd(), stream);
}

// Stages entries and records for one call.  Of{cigar, n_cigar}(e): element e of the scan's input, a tuple (Of::Tuple) that begins with
// cig_bases.  n_items: the caller's queries or ranges, for which the status words and the reduction's temporary are sized as well.
// behind(): what else the caller launches under `timer` once k_lift_check and its reduction are queued.  Returns NTS_ENOMEM while
// nothing is queued yet; behind that NTS_OK with the stream's state in e_run, the copy of the smallest offending chain into *worst
// queued and the stream NOT synchronised: entries and records are sources of asynchronous copies, so the caller synchronises once
// whatever happened.
template <class Of, class Behind>
int cig_index_stage(nts_ctx* ctx, const char* timer, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains, uint64_t n_items,
                    uint32_t* worst, CigIndex& ix, hipError_t& e_run, Behind behind)
{
  constexpr size_t NP = rocprim::tuple_size<typename Of::Tuple>::value;
  const auto columns = std::make_index_sequence<NP>();
  const uint64_t lanes = n_cigar + n_chains, most = std::max(lanes, n_items);
  NTS_WS(d_cigar, uint64_t*, "cigx_cigar", std::max<uint64_t>(n_cigar, 1) * 8);
  NTS_WS(d_chains, nts_cig_chain*, "cigx_chains", std::max<uint64_t>(n_chains, 1) * sizeof(nts_cig_chain));
  NTS_WS(d_prefixes, uint64_t*, "cigx_prefixes", NP * (n_cigar + 1) * 8);
  NTS_WS(d_status, uint32_t*, "cigx_status", std::max<uint64_t>(most, 1) * 4);
  NTS_WS(d_worst, uint32_t*, "cigx_worst", 2 * 4);
  ix = { d_cigar, d_chains, d_prefixes, n_cigar + 1, d_status, d_worst, nullptr, 0 };
  e_run = hipSuccess;
  if (n_cigar) e_run = hipMemcpyAsync(d_cigar, cigar, n_cigar * 8, hipMemcpyHostToDevice, ctx->stream);
  if (e_run == hipSuccess && n_chains) e_run = hipMemcpyAsync(d_chains, chains, n_chains * sizeof(nts_cig_chain), hipMemcpyHostToDevice, ctx->stream);
  if (e_run == hipSuccess) {
    ScopedTimer t(ctx, timer, true);
    size_t tmp_s = 0;
    e_run = cig_index_scan<Of>(nullptr, tmp_s, ix, n_cigar, ctx->stream, columns);
    if (e_run == hipSuccess) e_run = rocprim::reduce(nullptr, ix.tmp_bytes, d_status, d_worst, SCRIPT_OK, most, ScriptMin(), ctx->stream);
    ix.tmp = e_run == hipSuccess ? ws_get(ctx, "ivs_tmp", std::max<size_t>(std::max(tmp_s, ix.tmp_bytes), 16)) : nullptr; // (once, behind both sizes)
    if (e_run == hipSuccess && !ix.tmp) e_run = hipErrorOutOfMemory;
    if (e_run == hipSuccess) e_run = cig_index_scan<Of>(ix.tmp, tmp_s, ix, n_cigar, ctx->stream, columns);
    if (e_run == hipSuccess && lanes) {
      NTS_LAUNCH(k_lift_check<CigOfPadded<Of>::value>, IVL_GRID(lanes), ix.cigar, n_cigar, ix.chains, n_chains, ix.column(0), ix.column(1), d_status);
      e_run = rocprim::reduce(ix.tmp, ix.tmp_bytes, d_status, d_worst, SCRIPT_OK, lanes, ScriptMin(), ctx->stream);
    }
    if (e_run == hipSuccess) behind();
  }
  if (e_run == hipSuccess && lanes) e_run = hipMemcpyAsync(worst, d_worst, 4, hipMemcpyDeviceToHost, ctx->stream);
  return NTS_OK;
}

// ---- the coordinate map of the chains' CIGARs (nts_cigar_lift; ntsynt_amd/assess.py block_lift) ----
// docs/design/04_23_block_lift.md.  Input: CIGAR entries and chain records as nts_cigar_build returns them, and queries {chain, side, pos}:
// an offset on side A (0) or B (1) of a chain.  The answer is the offset on the other side and the entry the position falls in.
//   1  cig_index_stage with the pair (A bases, B bases) alone: the columns PA and PB (timer "lift_scan").
//   2  k_cig_lift: one lane per query; validates it, finds with an upper-bound binary search over Psrc the entry that holds pos and
//      stores one 32 B hit; an invalid query stores nothing but its own index in its status word, a second minimum reduction names the
//      smallest (timer "lift_search").
// No atomic, no launch per chain or query, no floating point, no host loop over entries or queries.

constexpr uint32_t LIFT_MAX_BASES_LOG2 = 63; // the global scan must not wrap
static_assert(sizeof(nts_lift_query) == 16 && sizeof(nts_lift_hit) == 32, "the C ABI's layout");

struct LiftBasesOf // element e of the scan's input: what entry e consumes; nothing behind the last entry
{
  using Tuple = CigBases;
  const uint64_t* cigar;
  uint64_t n_cigar;
  __host__ __device__ Tuple operator()(uint64_t e) const { return e < n_cigar ? cig_bases(cigar[e]) : Tuple(0, 0); }
};

__global__ __launch_bounds__(256) void k_cig_lift(const uint64_t* __restrict__ cigar, uint64_t n_cigar, const nts_cig_chain* __restrict__ chains,
                                                  uint64_t n_chains, const uint64_t* __restrict__ PA, const uint64_t* __restrict__ PB,
                                                  const nts_lift_query* __restrict__ queries, uint64_t n_queries, nts_lift_hit* __restrict__ hits,
                                                  uint32_t* __restrict__ status)
{
  const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (g >= n_queries) return;
  const nts_lift_query q = queries[g];
  nts_cig_chain ch;
  if (!cig_chain_of(chains, n_chains, q.chain, q.side, ch)) {
    status[g] = (uint32_t)g;
    return;
  }
  const uint64_t first = ch.first, n = ch.n_cig;
  const uint64_t len_src = q.side ? ch.len_b : ch.len_a, len_oth = q.side ? ch.len_a : ch.len_b;
  // (a chain without entries holds no base: every index below is <= first + n <= n_cigar)
  if (cig_chain_beyond(ch, n_cigar) || q.pos > len_src || (q.pos < len_src && n == 0)) {
    status[g] = (uint32_t)g;
    return;
  }
  status[g] = SCRIPT_OK;
  if (q.pos == len_src) { // the end of a half-open interval
    hits[g] = { len_oth, first + n, 0, 0u, 0u };
    return;
  }
  const uint64_t* __restrict__ P = q.side ? PB : PA;
  const uint64_t* __restrict__ O = q.side ? PA : PB;
  const uint64_t base = P[first];
  const uint64_t lo = cig_entry_of(P, base, first, first + n, q.pos);
  const uint64_t code = cigar[lo] & 15u; // (first <= lo < first + n <= n_cigar)
  const uint64_t off = q.pos - (P[lo] - base);
  hits[g] = { O[lo] - O[first] + (code == CIG_EQ || code == CIG_X ? off : 0), lo, off, (uint32_t)code, 0u };
}

int cigar_lift_run(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains, const nts_lift_query* queries,
                   uint64_t n_queries, nts_lift_hit* hits)
{
  if (const int rc = cig_chains_check(ctx, "nts_cigar_lift", LIFT_MAX_BASES_LOG2, false, chains, n_chains, n_cigar, [](uint64_t, auto) { return NTS_OK; })) return rc;
  // (its own buffers first: while nothing is queued, a request that fails may still return at once)
  NTS_WS(d_queries, nts_lift_query*, "lift_queries", std::max<uint64_t>(n_queries, 1) * sizeof(nts_lift_query));
  NTS_WS(d_hits, nts_lift_hit*, "lift_hits", std::max<uint64_t>(n_queries, 1) * sizeof(nts_lift_hit));
  nts_lift_hit* host_hits = n_queries ? (nts_lift_hit*)malloc(n_queries * sizeof(nts_lift_hit)) : nullptr; // (the caller's array is written only on success)
  if (n_queries && !host_hits) return fail(ctx, NTS_ENOMEM, "nts_cigar_lift: no host memory for the hits");
  uint32_t worst[2] = { SCRIPT_OK, SCRIPT_OK }; // the smallest offending chain, the smallest offending query
  CigIndex ix;
  hipError_t e_run;
  if (const int rc = cig_index_stage<LiftBasesOf>(ctx, "lift_scan", cigar, n_cigar, chains, n_chains, n_queries, &worst[0], ix, e_run, [] {})) {
    free(host_hits);
    return rc;
  }
  if (e_run == hipSuccess && n_queries)
    e_run = hipMemcpyAsync(d_queries, queries, n_queries * sizeof(nts_lift_query), hipMemcpyHostToDevice, ctx->stream);
  if (e_run == hipSuccess && n_queries) { // (no query: nothing more is launched)
    ScopedTimer t(ctx, "lift_search", true);
    NTS_LAUNCH(k_cig_lift, IVL_GRID(n_queries), ix.cigar, n_cigar, ix.chains, n_chains, ix.column(0), ix.column(1), (const nts_lift_query*)d_queries, n_queries,
               d_hits, ix.status);
    e_run = rocprim::reduce(ix.tmp, ix.tmp_bytes, ix.status, ix.worst + 1, SCRIPT_OK, n_queries, ScriptMin(), ctx->stream);
  }
  if (e_run == hipSuccess) e_run = hipGetLastError();
  if (e_run == hipSuccess && n_queries) e_run = hipMemcpyAsync(&worst[1], ix.worst + 1, 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e_run == hipSuccess && n_queries) e_run = hipMemcpyAsync(host_hits, d_hits, n_queries * sizeof(nts_lift_hit), hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t e_sync = hipStreamSynchronize(ctx->stream); // (whatever happened: the caller's arrays were sources of asynchronous copies)
  const bool good = e_run == hipSuccess && e_sync == hipSuccess && worst[0] == SCRIPT_OK && worst[1] == SCRIPT_OK;
  if (good && n_queries) memcpy(hits, host_hits, n_queries * sizeof(nts_lift_hit));
  free(host_hits);
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  if (worst[0] != SCRIPT_OK) return fail(ctx, NTS_EINVAL, "nts_cigar_lift: the entries of chain " + std::to_string(worst[0]) + " are no CIGAR of its lengths");
  if (worst[1] != SCRIPT_OK) return fail(ctx, NTS_EINVAL, "nts_cigar_lift: query " + std::to_string(worst[1]) + " is outside its chain");
  return NTS_OK;
}

// ---- the alignment counts of ranges of the chains' CIGARs (nts_cigar_lift_stats; ntsynt_amd/assess.py block_lift_identity) ----
// docs/design/04_25_lift_identity.md.  Input: CIGAR entries and chain records as for nts_cigar_lift, and ranges {chain, side, lo, hi}: the
// source bases lo .. hi - 1 of one side of a chain.  The answer counts the chain's columns from the column of base lo to the column of
// base hi - 1: =, X, the columns that consume the source only, the columns that consume the other side only, the runs of either gap
// kind, and the lifted span [oth_lo, oth_hi) on the other side.
//   1  cig_index_stage with (A bases, B bases, X columns, D columns, I heads | D heads << 32): five columns; a head is an entry whose
//      predecessor in the array has another code, or entry 0.  = columns are A - X - D, I columns B - A + D (timer "lift_stats_scan").
//   2  k_cig_lift_stats: one lane per range; validates it, finds the entries of base lo and of base hi - 1 with two upper-bound
//      binary searches over Psrc, takes the whole entries between them as prefix differences and the two partial entries from their
//      offsets, and stores one 64 B record; an invalid range stores nothing but its own index in its status word, a second minimum
//      reduction names the smallest (timer "lift_stats_search").
// No atomic, no launch per chain or range, no floating point, no host loop over entries or ranges.

using LiftStatTuple = rocprim::tuple<uint64_t, uint64_t, uint64_t, uint64_t, uint64_t>; // A bases, B bases, X columns, D columns, I heads | D heads << 32
static_assert(sizeof(nts_lift_range) == 24 && sizeof(nts_lift_stats) == 64, "the C ABI's layout");

struct LiftStatOf // element e of the scan's input: what entry e adds; nothing behind the last entry
{
  using Tuple = LiftStatTuple;
  const uint64_t* cigar;
  uint64_t n_cigar;
  __host__ __device__ Tuple operator()(uint64_t e) const
  {
    if (e >= n_cigar) return Tuple(0, 0, 0, 0, 0);
    const uint64_t v = cigar[e], code = v & 15u, len = v >> 4;
    const CigBases ab = cig_bases(v);
    const bool head = e == 0 || (cigar[e - 1] & 15u) != code;
    return Tuple(rocprim::get<0>(ab), rocprim::get<1>(ab), code == CIG_X ? len : 0, code == CIG_D ? len : 0,
                 !head ? 0 : code == CIG_I ? 1ull : code == CIG_D ? 1ull << 32 : 0); // (at most n_cigar < 2^32 heads of a kind: no carry between the halves)
  }
};

__global__ __launch_bounds__(256) void k_cig_lift_stats(const uint64_t* __restrict__ cigar, uint64_t n_cigar, const nts_cig_chain* __restrict__ chains,
                                                        uint64_t n_chains, const uint64_t* __restrict__ PA, const uint64_t* __restrict__ PB,
                                                        const uint64_t* __restrict__ PX, const uint64_t* __restrict__ PD, const uint64_t* __restrict__ PH,
                                                        const nts_lift_range* __restrict__ ranges, uint64_t n_ranges, nts_lift_stats* __restrict__ stats,
                                                        uint32_t* __restrict__ status)
{
  const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (g >= n_ranges) return;
  const nts_lift_range r = ranges[g];
  nts_cig_chain ch;
  if (!cig_chain_of(chains, n_chains, r.chain, r.side, ch)) {
    status[g] = (uint32_t)g;
    return;
  }
  const uint64_t first = ch.first, n = ch.n_cig;
  const uint64_t len_src = r.side ? ch.len_b : ch.len_a;
  // (a chain without entries holds no base: every index below is <= first + n <= n_cigar)
  if (cig_chain_beyond(ch, n_cigar) || n == 0 || r.lo >= r.hi || r.hi > len_src) {
    status[g] = (uint32_t)g;
    return;
  }
  status[g] = SCRIPT_OK;
  const uint64_t* __restrict__ P = r.side ? PB : PA;
  const uint64_t* __restrict__ O = r.side ? PA : PB;
  const uint64_t base = P[first], last = r.hi - 1u;
  const uint64_t e_lo = cig_entry_of(P, base, first, first + n, r.lo);
  const uint64_t e_hi = cig_entry_of(P, base, e_lo, first + n, last); // (P[e_lo] - base <= lo <= hi - 1: the entry of base hi - 1 is e_lo or lies behind it)
  // first <= e_lo <= e_hi < first + n <= n_cigar: cigar[e_lo], cigar[e_hi]; the prefixes at e_lo + 1 and e_hi + 1 <= first + n <= n_cigar
  const uint64_t v_lo = cigar[e_lo], v_hi = cigar[e_hi];
  const uint64_t code_lo = v_lo & 15u, code_hi = v_hi & 15u;
  const uint64_t off_lo = r.lo - (P[e_lo] - base), off_hi = last - (P[e_hi] - base);
  const uint64_t src_only = r.side ? CIG_I : CIG_D;
  uint64_t eq = 0, x = 0, src_gap = 0, oth_gap = 0;
  if (e_lo == e_hi) { // off_hi - off_lo + 1 columns of that entry's kind
    const uint64_t cols = off_hi - off_lo + 1u;
    if (code_lo == CIG_EQ) eq = cols;
    else if (code_lo == CIG_X) x = cols;
    else src_gap = cols;
  } else { // the rest of e_lo, the whole entries e_lo + 1 .. e_hi - 1 as prefix differences, the first off_hi + 1 columns of e_hi
    const uint64_t a = PA[e_hi] - PA[e_lo + 1u], b = PB[e_hi] - PB[e_lo + 1u], mx = PX[e_hi] - PX[e_lo + 1u], md = PD[e_hi] - PD[e_lo + 1u];
    const uint64_t meq = a - mx - md, mi = b - meq - mx;
    const uint64_t head = (v_lo >> 4) - off_lo, tail = off_hi + 1u;
    eq = meq + (code_lo == CIG_EQ ? head : 0) + (code_hi == CIG_EQ ? tail : 0);
    x = mx + (code_lo == CIG_X ? head : 0) + (code_hi == CIG_X ? tail : 0);
    src_gap = (r.side ? mi : md) + (code_lo == src_only ? head : 0) + (code_hi == src_only ? tail : 0);
    oth_gap = r.side ? md : mi; // (e_lo and e_hi consume the source: a column of the other side alone lies in a whole entry between them)
  }
  const uint64_t heads = PH[e_hi + 1u] - PH[e_lo + 1u]; // the heads among the entries (e_lo, e_hi]: I in the low half, D in the high
  const uint32_t i_heads = (uint32_t)heads, d_heads = (uint32_t)(heads >> 32);
  const uint32_t opens = code_lo == src_only ? 1u : 0u; // (a run cut by the range's start counts once)
  const bool both_lo = code_lo == CIG_EQ || code_lo == CIG_X, both_hi = code_hi == CIG_EQ || code_hi == CIG_X;
  stats[g] = { O[e_lo] - O[first] + (both_lo ? off_lo : 0), O[e_hi] - O[first] + (both_hi ? off_hi + 1u : 0), eq, x, src_gap, oth_gap,
               (r.side ? i_heads : d_heads) + opens, r.side ? d_heads : i_heads, 0 };
}

int cigar_lift_stats_run(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains, const nts_lift_range* ranges,
                         uint64_t n_ranges, nts_lift_stats* stats)
{
  if (const int rc = cig_chains_check(ctx, "nts_cigar_lift_stats", LIFT_MAX_BASES_LOG2, false, chains, n_chains, n_cigar, [](uint64_t, auto) { return NTS_OK; })) return rc;
  // (its own buffers first: while nothing is queued, a request that fails may still return at once)
  NTS_WS(d_ranges, nts_lift_range*, "lstat_ranges", std::max<uint64_t>(n_ranges, 1) * sizeof(nts_lift_range));
  NTS_WS(d_stats, nts_lift_stats*, "lstat_stats", std::max<uint64_t>(n_ranges, 1) * sizeof(nts_lift_stats));
  nts_lift_stats* host_stats = n_ranges ? (nts_lift_stats*)malloc(n_ranges * sizeof(nts_lift_stats)) : nullptr; // (the caller's array is written only on success)
  if (n_ranges && !host_stats) return fail(ctx, NTS_ENOMEM, "nts_cigar_lift_stats: no host memory for the records");
  uint32_t worst[2] = { SCRIPT_OK, SCRIPT_OK }; // the smallest offending chain, the smallest offending range
  CigIndex ix; // columns PA, PB, PX, PD, PH
  hipError_t e_run;
  if (const int rc = cig_index_stage<LiftStatOf>(ctx, "lift_stats_scan", cigar, n_cigar, chains, n_chains, n_ranges, &worst[0], ix, e_run, [] {})) {
    free(host_stats);
    return rc;
  }
  if (e_run == hipSuccess && n_ranges) e_run = hipMemcpyAsync(d_ranges, ranges, n_ranges * sizeof(nts_lift_range), hipMemcpyHostToDevice, ctx->stream);
  if (e_run == hipSuccess && n_ranges) { // (no range: nothing more is launched)
    ScopedTimer t(ctx, "lift_stats_search", true);
    NTS_LAUNCH(k_cig_lift_stats, IVL_GRID(n_ranges), ix.cigar, n_cigar, ix.chains, n_chains, ix.column(0), ix.column(1), ix.column(2), ix.column(3), ix.column(4),
               (const nts_lift_range*)d_ranges, n_ranges, d_stats, ix.status);
    e_run = rocprim::reduce(ix.tmp, ix.tmp_bytes, ix.status, ix.worst + 1, SCRIPT_OK, n_ranges, ScriptMin(), ctx->stream);
  }
  if (e_run == hipSuccess) e_run = hipGetLastError();
  if (e_run == hipSuccess && n_ranges) e_run = hipMemcpyAsync(&worst[1], ix.worst + 1, 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e_run == hipSuccess && n_ranges) e_run = hipMemcpyAsync(host_stats, d_stats, n_ranges * sizeof(nts_lift_stats), hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t e_sync = hipStreamSynchronize(ctx->stream); // (whatever happened: the caller's arrays were sources of asynchronous copies)
  const bool good = e_run == hipSuccess && e_sync == hipSuccess && worst[0] == SCRIPT_OK && worst[1] == SCRIPT_OK;
  if (good && n_ranges) memcpy(stats, host_stats, n_ranges * sizeof(nts_lift_stats));
  free(host_stats);
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  if (worst[0] != SCRIPT_OK)
    return fail(ctx, NTS_EINVAL, "nts_cigar_lift_stats: the entries of chain " + std::to_string(worst[0]) + " are no CIGAR of its lengths");
  if (worst[1] != SCRIPT_OK) return fail(ctx, NTS_EINVAL, "nts_cigar_lift_stats: range " + std::to_string(worst[1]) + " is outside its chain");
  return NTS_OK;
}

// ---- the cg:Z: and cs:Z: texts of the chains' CIGARs (nts_cigar_text; ntsynt_amd/assess.py block_alignments with cs) ----
// docs/design/04_26_block_paf_cs.md.  Input: CIGAR entries and chain records as nts_cigar_build returns them, the chains tiling the entries,
// and per chain a span that places it in a record of genome a (target, forwards) and of genome b (query, forwards or backwards and
// complemented).  A TOKEN is what one entry gives a text: cg "<len><letter>"; cs ":<len>" for =, "*tq" per column for X, "-" / "+" and
// the bases for D / I.  Every token has at least 2 bytes.
//   1  cig_index_stage with (A bases, B bases, cg bytes, cs bytes): four columns; behind its check, k_cig_text_firsts reads the byte
//      prefixes at every chain's first entry (timer "cigar_text_scan").  The chains tile the entries (host check), so a chain's text
//      is one byte range.
//   2  k_cig_text<kind>: one lane per aligned 4-byte word of the text; an upper-bound binary search over the byte prefix finds the entry
//      of the word's first byte, the lane walks on over the at most three further entries a word touches, composes four bytes in a
//      register and stores one dword (timer "cigar_text_emit").  A base byte finds its chain by a search over the chains' first
//      entries and reads one code at the chain's base address plus the A or B prefix difference.  No lane loops over columns.
// No atomic, no launch per chain or entry, no floating point, no host loop over entries.

using CigTextTuple = rocprim::tuple<uint64_t, uint64_t, uint64_t, uint64_t>; // A bases, B bases, cg bytes, cs bytes
constexpr uint32_t CIG_TEXT_MAX_BASES_LOG2 = 62; // cs bytes <= 3 X + D + I + 20 n_cigar <= A + B + min(A, B) + 20 n_cigar: inside 64 bits
constexpr uint32_t CIG_TEXT_CG = 0, CIG_TEXT_CS = 1;
static_assert(sizeof(nts_cig_span) == 32, "the C ABI's layout");

__device__ const uint64_t CIG_POW10[20] = { 1ull,
                                            10ull,
                                            100ull,
                                            1000ull,
                                            10000ull,
                                            100000ull,
                                            1000000ull,
                                            10000000ull,
                                            100000000ull,
                                            1000000000ull,
                                            10000000000ull,
                                            100000000000ull,
                                            1000000000000ull,
                                            10000000000000ull,
                                            100000000000000ull,
                                            1000000000000000ull,
                                            10000000000000000ull,
                                            100000000000000000ull,
                                            1000000000000000000ull,
                                            10000000000000000000ull };

// len / 10^j without a division by a runtime value (the compiler expands one through floating-point reciprocals): for a dividend below
// 2^60 and l = ceil(log2 10^j), M = floor(2^(60 + l) / 10^j) + 1 gives floor(len / 10^j) = (len M) >> (60 + l) exactly (Granlund and
// Montgomery 1994, theorem 4.2); the table holds M and 60 + l - 64, the shift of the product's upper half, for j = 1 .. 18
struct CigPow10Inverse
{
  uint64_t mul;
  uint32_t shift;
};
__device__ const CigPow10Inverse CIG_POW10_INVERSE[18] = {
  { 1844674407370955162ull, 0u },  { 1475739525896764130ull, 3u },  { 1180591620717411304ull, 6u },  { 1888946593147858086ull, 10u },
  { 1511157274518286469ull, 13u }, { 1208925819614629175ull, 16u }, { 1934281311383406680ull, 20u }, { 1547425049106725344ull, 23u },
  { 1237940039285380275ull, 26u }, { 1980704062856608440ull, 30u }, { 1584563250285286752ull, 33u }, { 1267650600228229402ull, 36u },
  { 2028240960365167043ull, 40u }, { 1622592768292133634ull, 43u }, { 1298074214633706908ull, 46u }, { 2076918743413931052ull, 50u },
  { 1661534994731144842ull, 53u }, { 1329227995784915873ull, 56u } };

// the decimal digit of weight 10^j of len < 2^60, j <= 18
__device__ __forceinline__ uint32_t cig_digit(uint64_t len, uint32_t j)
{
  uint64_t q = len;
  if (j > 0) {
    const CigPow10Inverse inv = CIG_POW10_INVERSE[(j <= 18u ? j : 18u) - 1u];
    q = __umul64hi(len, inv.mul) >> inv.shift;
  }
  return (uint32_t)(q - (q / 10u) * 10u); // (by the constant 10: a multiplication)
}

// the decimal digits of v, 1 for 0: t = floor(bits * log10(2)) is the digit count or one below it (bits <= 64: t <= 19)
__device__ __forceinline__ uint32_t cig_digits(uint64_t v)
{
  const uint32_t bits = 64u - (uint32_t)__builtin_clzll(v | 1u);
  const uint32_t t = (bits * 1233u) >> 12;
  return t + (v >= CIG_POW10[t] ? 1u : 0u) + (v == 0 ? 1u : 0u);
}

struct CigTextChain // a chain as the emit kernel reads it: where its bases lie in the code arrays
{
  uint64_t first, at_a, at_b, len_a, len_b; // at_*: the index into d_code (PAD included) of the chain's first base of that side
  uint32_t flags, pad;
};
static_assert(sizeof(CigTextChain) == 48, "six 8-byte words");

struct CigTextOf // element e of the scan's input: what entry e consumes and how long its two tokens are; nothing behind the last entry
{
  using Tuple = CigTextTuple;
  const uint64_t* cigar;
  uint64_t n_cigar;
  __device__ Tuple operator()(uint64_t e) const
  {
    if (e >= n_cigar) return Tuple(0, 0, 0, 0);
    const uint64_t v = cigar[e], code = v & 15u, len = v >> 4;
    const CigBases ab = cig_bases(v);
    const bool both = code == CIG_EQ || code == CIG_X, gap = code == CIG_I || code == CIG_D;
    const uint64_t d = cig_digits(len);
    return Tuple(rocprim::get<0>(ab), rocprim::get<1>(ab), both || gap ? d + 1u : 0,
                 code == CIG_EQ ? d + 1u : code == CIG_X ? 3u * len : gap ? len + 1u : 0); // (len < 2^60: 3 len does not wrap)
  }
};

// lane c <= n_chains: where chain c's texts begin, the texts' lengths for c = n_chains
__global__ __launch_bounds__(256) void k_cig_text_firsts(const nts_cig_chain* __restrict__ chains, uint64_t n_chains, uint64_t n_cigar,
                                                         const uint64_t* __restrict__ PG, const uint64_t* __restrict__ PS, uint64_t* __restrict__ cg_first,
                                                         uint64_t* __restrict__ cs_first)
{
  const uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (c > n_chains) return;
  uint64_t f = c < n_chains ? chains[c].first : n_cigar;
  if (f > n_cigar) f = n_cigar; // (the host refused this before the launch: a lane still reads nothing outside the prefixes)
  cg_first[c] = PG[f];
  cs_first[c] = PS[f];
}

// the letter of the base idx of one side of a chain: 'n' for a code that is no base, '?' -- never seen in a text -- instead of a load
// outside the chain or the code array (the chain check and the host's span checks leave none)
__device__ __forceinline__ uint32_t cig_text_base(const uint8_t* __restrict__ code, uint64_t size, uint64_t at, uint64_t idx, uint64_t len, bool backwards)
{
  if (idx >= len || (backwards ? idx > at : idx >= size - at)) return '?';
  const uint64_t where = backwards ? at - idx : at + idx;
  if (where < PAD || where >= size - PAD) return '?';
  uint32_t c = code[where];
  if (c >= nts::CODE_INVALID) return 'n';
  if (backwards) c = 3u - c;
  return (0x74676361u >> (8u * c)) & 255u; // "acgt"
}

template <uint32_t KIND>
__global__ __launch_bounds__(256) void k_cig_text(const uint64_t* __restrict__ cigar, uint64_t n_cigar, const CigTextChain* __restrict__ chains,
                                                  uint64_t n_chains, const uint64_t* __restrict__ PA, const uint64_t* __restrict__ PB,
                                                  const uint64_t* __restrict__ P, const uint8_t* __restrict__ code_a, uint64_t size_a,
                                                  const uint8_t* __restrict__ code_b, uint64_t size_b, uint32_t* __restrict__ out, uint64_t n_words)
{
  const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (w >= n_words || n_cigar == 0) return;
  const uint64_t total = P[n_cigar], o = 4u * w;
  uint64_t e = cig_last_at_or_before(n_cigar, o, [P](uint64_t i) { return P[i]; }); // the entry of the word's first byte (P[0] = 0 <= o)
  uint64_t p0 = P[e], p1 = P[e + 1u]; // (e < n_cigar)
  uint64_t v = cigar[e];
  uint32_t digits = cig_digits(v >> 4);
  uint64_t chain_of = ~0ull; // the entry whose chain `ch` is
  CigTextChain ch = {};
  uint32_t word = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    const uint64_t at = o + k;
    if (at >= total) break;                  // (the padding of the last word stays 0)
    while (at >= p1 && e + 1u < n_cigar) { // the next entry: a token has at least 2 bytes, so at most three steps per word
      ++e;
      p0 = p1;
      p1 = P[e + 1u];
      v = cigar[e];
      digits = cig_digits(v >> 4);
    }
    const uint64_t off = at - p0, len = v >> 4;
    const uint32_t code = (uint32_t)(v & 15u);
    uint32_t byte;
    if (KIND == CIG_TEXT_CG || code == CIG_EQ) {
      const uint64_t lead = KIND == CIG_TEXT_CG ? 0u : 1u, i = off - lead; // cs: ':' in front of the digits
      if (off < lead) byte = ':';
      else if (i < digits) byte = '0' + cig_digit(len, digits - 1u - (uint32_t)i); // (len / 10^(digits - 1 - i)) % 10
      else byte = code == CIG_I ? 'I' : code == CIG_D ? 'D' : code == CIG_EQ ? '=' : 'X';
    } else {
      const bool is_x = code == CIG_X;
      const uint64_t column = is_x ? off / 3u : off - 1u;
      const uint32_t part = is_x ? (uint32_t)(off % 3u) : (off == 0 ? 0u : code == CIG_D ? 1u : 2u); // 0: the sign, 1: a target base, 2: a query base
      if (part == 0) {
        byte = is_x ? '*' : code == CIG_D ? '-' : '+';
      } else {
        if (chain_of != e) { // the last chain with first <= e (chains[0].first = 0; empty chains in front of it share its first)
          ch = chains[cig_last_at_or_before(n_chains, e, [chains](uint64_t c) { return chains[c].first; })];
          chain_of = e;
        }
        const uint64_t f = ch.first <= e ? ch.first : e;
        byte = part == 1u ? cig_text_base(code_a, size_a, ch.at_a, PA[e] - PA[f] + column, ch.len_a, false)
                          : cig_text_base(code_b, size_b, ch.at_b, PB[e] - PB[f] + column, ch.len_b, (ch.flags & NTS_CIG_B_BACKWARDS) != 0);
      }
    }
    word |= byte << (8u * k);
  }
  out[w] = word;
}

int cigar_text_run(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains, const nts_genome* a,
                   const nts_genome* b, const nts_cig_span* spans, uint8_t** cg, uint64_t* cg_first, uint8_t** cs, uint64_t* cs_first)
{
  const bool with_cs = spans != nullptr;
  std::vector<CigTextChain> placed(with_cs ? n_chains : 0);
  auto place = [&](uint64_t c, auto who) -> int { // chain c's span, behind the checks of its record
    if (!with_cs) return NTS_OK;
    const nts_cig_chain& ch = chains[c];
    const nts_cig_span& sp = spans[c];
    if (sp.flags & ~NTS_CIG_B_BACKWARDS) return fail(ctx, NTS_EINVAL, who() + " has unknown flag bits");
    if (sp.rec_a >= a->n_rec || sp.rec_b >= b->n_rec) return fail(ctx, NTS_EINVAL, who() + " names a record outside its genome");
    const uint64_t rl_a = a->rec_len[sp.rec_a], rl_b = b->rec_len[sp.rec_b];
    const bool backwards = (sp.flags & NTS_CIG_B_BACKWARDS) != 0;
    bool inside = sp.pos_a <= rl_a && ch.len_a <= rl_a - sp.pos_a;
    if (ch.len_b == 0) inside = inside && sp.pos_b <= rl_b;
    else if (backwards) inside = inside && sp.pos_b < rl_b && ch.len_b <= sp.pos_b + 1u;
    else inside = inside && sp.pos_b <= rl_b && ch.len_b <= rl_b - sp.pos_b;
    if (!inside) return fail(ctx, NTS_EINVAL, who() + ": its span lies outside its record");
    placed[c] = { ch.first, PAD + a->rec_off[sp.rec_a] + sp.pos_a, PAD + b->rec_off[sp.rec_b] + sp.pos_b, ch.len_a, ch.len_b, sp.flags, 0u };
    return NTS_OK;
  };
  if (const int rc = cig_chains_check(ctx, "nts_cigar_text", CIG_TEXT_MAX_BASES_LOG2, true, chains, n_chains, n_cigar, place)) return rc;
  if (n_cigar == 0) { // (nothing is launched: every text is empty)
    *cg = nullptr;
    memset(cg_first, 0, (n_chains + 1) * 8);
    if (with_cs) {
      *cs = nullptr;
      memset(cs_first, 0, (n_chains + 1) * 8);
    }
    return NTS_OK;
  }
  // (its own buffers first: while nothing is queued, a request that fails may still return at once)
  NTS_WS(d_placed, CigTextChain*, "cigt_placed", n_chains * sizeof(CigTextChain));
  NTS_WS(d_first, uint64_t*, "cigt_first", 2 * (n_chains + 1) * 8);
  std::vector<uint64_t> host_first(2 * (n_chains + 1)); // (the caller's arrays are written only when the call succeeds)
  uint32_t worst = SCRIPT_OK;
  CigIndex ix; // columns PA, PB, PG (cg bytes), PS (cs bytes)
  hipError_t e_run;
  auto firsts = [&] {
    NTS_LAUNCH(k_cig_text_firsts, IVL_GRID(n_chains + 1), ix.chains, n_chains, n_cigar, ix.column(2), ix.column(3), d_first, d_first + (n_chains + 1));
  };
  if (const int rc = cig_index_stage<CigTextOf>(ctx, "cigar_text_scan", cigar, n_cigar, chains, n_chains, 0, &worst, ix, e_run, firsts)) return rc;
  if (e_run == hipSuccess) e_run = hipGetLastError();
  if (e_run == hipSuccess && with_cs) e_run = hipMemcpyAsync(d_placed, placed.data(), n_chains * sizeof(CigTextChain), hipMemcpyHostToDevice, ctx->stream);
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(host_first.data(), d_first, 2 * (n_chains + 1) * 8, hipMemcpyDeviceToHost, ctx->stream);
  hipError_t e_sync = hipStreamSynchronize(ctx->stream); // (whatever happened: the caller's arrays were sources of asynchronous copies)
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  if (worst != SCRIPT_OK) return fail(ctx, NTS_EINVAL, "nts_cigar_text: the entries of chain " + std::to_string(worst) + " are no CIGAR of its lengths");
  const uint64_t bytes_cg = host_first[n_chains], bytes_cs = with_cs ? host_first[2 * n_chains + 1] : 0;
  if (bytes_cg > 0xFFFFFFFFull || bytes_cs > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_cigar_text: a text of 2^32 bytes or more");
  const uint64_t words_cg = (bytes_cg + 3) / 4, words_cs = (bytes_cs + 3) / 4; // (the device buffers are padded to whole words)
  NTS_WS(d_cg, uint32_t*, "cigt_cg", std::max<uint64_t>(words_cg, 1) * 4);
  NTS_WS(d_cs, uint32_t*, "cigt_cs", std::max<uint64_t>(words_cs, 1) * 4);
  uint8_t* host_cg = (uint8_t*)malloc(std::max<uint64_t>(bytes_cg, 1));
  uint8_t* host_cs = with_cs ? (uint8_t*)malloc(std::max<uint64_t>(bytes_cs, 1)) : nullptr;
  if (!host_cg || (with_cs && !host_cs)) {
    free(host_cg);
    free(host_cs);
    return fail(ctx, NTS_ENOMEM, "nts_cigar_text: no host memory for the texts");
  }
  {
    ScopedTimer t(ctx, "cigar_text_emit", true);
    NTS_LAUNCH(k_cig_text<CIG_TEXT_CG>, IVL_GRID(words_cg), ix.cigar, n_cigar, (const CigTextChain*)nullptr, (uint64_t)0, ix.column(0), ix.column(1),
               ix.column(2), (const uint8_t*)nullptr, (uint64_t)0, (const uint8_t*)nullptr, (uint64_t)0, d_cg, words_cg);
    if (with_cs)
      NTS_LAUNCH(k_cig_text<CIG_TEXT_CS>, IVL_GRID(words_cs), ix.cigar, n_cigar, (const CigTextChain*)d_placed, n_chains, ix.column(0), ix.column(1),
                 ix.column(3), (const uint8_t*)a->d_code, a->n + 2 * PAD, (const uint8_t*)b->d_code, b->n + 2 * PAD, d_cs, words_cs);
  }
  e_run = hipGetLastError();
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(host_cg, d_cg, bytes_cg, hipMemcpyDeviceToHost, ctx->stream);
  if (e_run == hipSuccess && with_cs && bytes_cs) e_run = hipMemcpyAsync(host_cs, d_cs, bytes_cs, hipMemcpyDeviceToHost, ctx->stream);
  e_sync = hipStreamSynchronize(ctx->stream);
  if (e_run != hipSuccess || e_sync != hipSuccess) {
    free(host_cg);
    free(host_cs);
  }
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  *cg = host_cg;
  memcpy(cg_first, host_first.data(), (n_chains + 1) * 8);
  if (with_cs) {
    *cs = host_cs;
    memcpy(cs_first, host_first.data() + (n_chains + 1), (n_chains + 1) * 8);
  }
  return NTS_OK;
}

// ---- one span and its counts per range and PAIR of chains (nts_cigar_lift_pairs; ntsynt_amd/assess.py lift_joined_table) ----
// docs/design/04_27_lift_joined.md.  Input: CIGAR entries and chain records as for nts_cigar_lift_stats, LINKS {chain, a0, b0} that place
// chains in the oriented coordinates of a pair -- pair_first[n_pairs + 1] cuts them into pairs, a pair's links ascend without overlap on
// both sides -- and ranges {pair, side, lo, hi}: the source bases lo .. hi - 1 of one side of a pair.  The answer counts the pair's
// columns from the column of the first base of the range that a chain holds to the column of the last one, the chains between the two
// whole, and the bases of the open stretches between the chains.
//   1  cig_index_stage with LiftStatOf's five columns; behind its check k_lpair_claim and k_lpair_twice find the chains that are linked
//      more than once, k_lpair_links -- one lane per link -- validates the link against the records and its predecessor in the pair and
//      writes its placement and the chain's whole totals, read from the entry prefixes; a minimum reduction names the smallest bad link,
//      ONE exclusive scan over n_links + 1 elements turns the totals into link prefixes (timer "lift_pairs_scan").
//   2  k_lpair_ranges: one lane per range; validates it, finds link_lo and link_hi with two binary searches over the pair's links and
//      the two entries with cig_entry_of, adds the partial head of link_lo, the whole chains between from the link prefixes and the
//      partial tail of link_hi, and stores one 128 B record; an invalid range stores nothing but its own index in its status word
//      (timer "lift_pairs_search").
// No atomic, no launch per pair, chain or range, no floating point, no host loop over links, ranges or entries.

static_assert(sizeof(nts_lift_link) == 24 && sizeof(nts_pair_range) == 24 && sizeof(nts_pair_stats) == 128, "the C ABI's layout");
constexpr uint64_t LPAIR_MAX_BASE = 1ull << 63;  // a link ends, and a range lies, in front of it
constexpr uint32_t LPAIR_TWICE = 0xFFFFFFFFu;    // "lpair_owner": the chain has more than one link

struct LpairPlace // a validated link as the range kernel reads it: where its chain's entries lie and what it occupies; n_cig = 0: a bad link
{
  uint64_t first, n_cig, a0, a1, b0, b1;
};
static_assert(sizeof(LpairPlace) == 48, "six 8-byte words");

struct LpairTotalsOf // element i of the link scan's input: the totals of link i's chain; nothing behind the last link
{
  using Tuple = LiftStatTuple; // A bases, B bases, X columns, D columns, I runs | D runs << 32 (the chain's own first entry opens one)
  const uint64_t* totals;      // five columns of n_links words
  uint64_t n_links;
  __host__ __device__ Tuple operator()(uint64_t i) const
  {
    if (i >= n_links) return Tuple(0, 0, 0, 0, 0);
    return Tuple(totals[i], totals[n_links + i], totals[2u * n_links + i], totals[3u * n_links + i], totals[4u * n_links + i]);
  }
};

// every link stores its index at its chain: one of a chain's links stays.  Several lanes may store different words to one owner[c]
// without an atomic: this relies on an aligned 32-bit store being written whole (one of the stored words stays, never a mixture) and on
// the kernel boundary between this kernel and k_lpair_twice, behind which every lane reads the word that stayed.
__global__ __launch_bounds__(256) void k_lpair_claim(const nts_lift_link* __restrict__ links, uint64_t n_links, uint64_t n_chains, uint32_t* __restrict__ owner)
{
  const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (g >= n_links) return;
  const uint32_t c = links[g].chain;
  if (c < n_chains) owner[c] = (uint32_t)g;
}

// a link that finds another one's index at its chain marks the chain (every writer stores the same word; a link that already reads the
// mark stores it again)
__global__ __launch_bounds__(256) void k_lpair_twice(const nts_lift_link* __restrict__ links, uint64_t n_links, uint64_t n_chains, uint32_t* __restrict__ owner)
{
  const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (g >= n_links) return;
  const uint32_t c = links[g].chain;
  if (c < n_chains && owner[c] != (uint32_t)g) owner[c] = LPAIR_TWICE;
}

__global__ __launch_bounds__(256) void k_lpair_links(const uint64_t* __restrict__ cigar, uint64_t n_cigar, const nts_cig_chain* __restrict__ chains,
                                                     uint64_t n_chains, const uint64_t* __restrict__ PA, const uint64_t* __restrict__ PB,
                                                     const uint64_t* __restrict__ PX, const uint64_t* __restrict__ PD, const uint64_t* __restrict__ PH,
                                                     const nts_lift_link* __restrict__ links, uint64_t n_links, const uint64_t* __restrict__ pair_first,
                                                     uint64_t n_pairs, const uint32_t* __restrict__ owner, LpairPlace* __restrict__ place,
                                                     uint64_t* __restrict__ totals, uint32_t* __restrict__ status)
{
  const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (g >= n_links) return;
  const nts_lift_link lk = links[g];
  nts_cig_chain ch;
  // (a chain without entries may not be linked; behind this first + n_cig <= n_cigar and n_cig >= 1)
  bool ok = lk.reserved == 0 && cig_chain_of(chains, n_chains, lk.chain, 0u, ch) && !cig_chain_beyond(ch, n_cigar) && ch.n_cig != 0;
  ok = ok && owner[lk.chain] != LPAIR_TWICE; // (lk.chain < n_chains)
  // (the host refused 2^63 bases or more: a0 + len_a does not wrap behind a0 < 2^63)
  ok = ok && lk.a0 < LPAIR_MAX_BASE && lk.b0 < LPAIR_MAX_BASE && ch.len_a < LPAIR_MAX_BASE - lk.a0 && ch.len_b < LPAIR_MAX_BASE - lk.b0;
  // its pair: the last with pair_first <= g (pair_first[0] = 0 <= g < n_links = pair_first[n_pairs]: n_pairs >= 1 here)
  const uint64_t p = cig_last_at_or_before(n_pairs, g, [pair_first](uint64_t i) { return pair_first[i]; });
  if (ok && g > pair_first[p]) { // the link in front of it in its pair; one that is bad itself is named instead
    const nts_lift_link pv = links[g - 1u];
    nts_cig_chain pc;
    if (cig_chain_of(chains, n_chains, pv.chain, 0u, pc) && pv.a0 < LPAIR_MAX_BASE && pv.b0 < LPAIR_MAX_BASE && pc.len_a < LPAIR_MAX_BASE - pv.a0 &&
        pc.len_b < LPAIR_MAX_BASE - pv.b0)
      ok = lk.a0 >= pv.a0 + pc.len_a && lk.b0 >= pv.b0 + pc.len_b;
  }
  uint64_t a = 0, b = 0, x = 0, d = 0, runs = 0;
  if (ok) {
    const uint64_t f = ch.first, end = f + ch.n_cig; // f < end <= n_cigar: the prefixes at f, f + 1 and end; cigar[f]
    a = PA[end] - PA[f];
    b = PB[end] - PB[f];
    x = PX[end] - PX[f];
    d = PD[end] - PD[f];
    const uint64_t code = cigar[f] & 15u;
    runs = PH[end] - PH[f + 1u] + (code == CIG_I ? 1ull : code == CIG_D ? 1ull << 32 : 0);
    place[g] = { f, ch.n_cig, lk.a0, lk.a0 + ch.len_a, lk.b0, lk.b0 + ch.len_b };
  } else {
    place[g] = { 0, 0, lk.a0, lk.a0, lk.b0, lk.b0 };
  }
  totals[g] = a;
  totals[n_links + g] = b;
  totals[2u * n_links + g] = x;
  totals[3u * n_links + g] = d;
  totals[4u * n_links + g] = runs;
  status[g] = ok ? SCRIPT_OK : (uint32_t)g;
}

__global__ __launch_bounds__(256) void k_lpair_ranges(const uint64_t* __restrict__ cigar, const uint64_t* __restrict__ PA, const uint64_t* __restrict__ PB,
                                                      const uint64_t* __restrict__ PX, const uint64_t* __restrict__ PD, const uint64_t* __restrict__ PH,
                                                      const LpairPlace* __restrict__ place, uint64_t n_links, const uint64_t* __restrict__ LA,
                                                      const uint64_t* __restrict__ LB, const uint64_t* __restrict__ LX, const uint64_t* __restrict__ LD,
                                                      const uint64_t* __restrict__ LH, const uint64_t* __restrict__ pair_first, uint64_t n_pairs,
                                                      const nts_pair_range* __restrict__ ranges, uint64_t n_ranges, nts_pair_stats* __restrict__ stats,
                                                      uint32_t* __restrict__ status)
{
  const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (g >= n_ranges) return;
  const nts_pair_range r = ranges[g];
  bool valid = r.pair < n_pairs && r.side <= 1u && r.lo < r.hi && r.hi < LPAIR_MAX_BASE;
  uint64_t l0 = 0, l1 = 0;
  if (valid) {
    l0 = pair_first[r.pair];
    l1 = pair_first[r.pair + 1u];
    valid = l0 <= l1 && l1 <= n_links; // (the host refused this before the launch: a lane still reads no link outside the array)
  }
  if (!valid) {
    status[g] = (uint32_t)g;
    return;
  }
  status[g] = SCRIPT_OK;
  const bool side = r.side != 0;
  auto s0 = [place, side](uint64_t i) { return side ? place[i].b0 : place[i].a0; };
  auto s1 = [place, side](uint64_t i) { return side ? place[i].b1 : place[i].a1; };
  // link_lo: the first link of the pair that ends behind lo; link_end: the first at or behind link_lo that starts at or behind hi.  Both
  // searches keep l0 <= lo_i <= hi_i <= l1 and read place[mid] with lo_i <= mid < hi_i, whatever the links hold.
  uint64_t lo_i = l0, hi_i = l1;
  while (lo_i < hi_i) {
    const uint64_t mid = lo_i + (hi_i - lo_i) / 2u;
    if (s1(mid) > r.lo) hi_i = mid;
    else lo_i = mid + 1u;
  }
  uint64_t link_lo = lo_i;
  hi_i = l1;
  while (lo_i < hi_i) {
    const uint64_t mid = lo_i + (hi_i - lo_i) / 2u;
    if (s0(mid) >= r.hi) hi_i = mid;
    else lo_i = mid + 1u;
  }
  uint64_t link_end = lo_i; // l0 <= link_lo <= link_end <= l1
  // a chain without a base of the source side holds no end column: it counts only between two chains that do.  The two loops are
  // linear in the src-empty links at either end of the run -- at most the pair's links; chains built from anchors hold bases of both
  // sides, so they step over nothing there (docs/design/04_27_lift_joined.md)
  while (link_lo < link_end && s1(link_lo) == s0(link_lo)) ++link_lo;
  while (link_end > link_lo && s1(link_end - 1u) == s0(link_end - 1u)) --link_end;
  nts_pair_stats out = {};
  if (link_lo == link_end) { // the range touches no chain
    stats[g] = out;
    return;
  }
  const uint64_t link_hi = link_end - 1u; // l0 <= link_lo <= link_hi < l1 <= n_links
  const LpairPlace p_lo = place[link_lo], p_hi = place[link_hi];
  if (p_lo.n_cig == 0 || p_hi.n_cig == 0) { // a bad link (the call fails on its status): no entry is read
    stats[g] = out;
    return;
  }
  const uint64_t* __restrict__ P = side ? PB : PA;
  const uint64_t* __restrict__ O = side ? PA : PB;
  const uint64_t s0_lo = side ? p_lo.b0 : p_lo.a0, s1_lo = side ? p_lo.b1 : p_lo.a1, s0_hi = side ? p_hi.b0 : p_hi.a0, s1_hi = side ? p_hi.b1 : p_hi.a1;
  const uint64_t o0_lo = side ? p_lo.a0 : p_lo.b0, o1_lo = side ? p_lo.a1 : p_lo.b1, o0_hi = side ? p_hi.a0 : p_hi.b0;
  const uint64_t src_lo = r.lo > s0_lo ? r.lo : s0_lo, src_hi = r.hi < s1_hi ? r.hi : s1_hi;
  const uint64_t f_lo = p_lo.first, end_lo = f_lo + p_lo.n_cig, f_hi = p_hi.first, end_hi = f_hi + p_hi.n_cig; // f < end <= n_cigar (k_lpair_links)
  const uint64_t base_lo = P[f_lo], base_hi = P[f_hi], u_lo = src_lo - s0_lo, u_last = src_hi - 1u - s0_hi;
  const uint64_t e_lo = cig_entry_of(P, base_lo, f_lo, end_lo, u_lo);
  const uint64_t e_hi = cig_entry_of(P, base_hi, link_lo == link_hi ? e_lo : f_hi, end_hi, u_last);
  // f_lo <= e_lo < end_lo and f_hi <= e_hi < end_hi, in one chain e_lo <= e_hi: cigar[e_lo], cigar[e_hi], the prefixes up to end <= n_cigar
  const uint64_t v_lo = cigar[e_lo], v_hi = cigar[e_hi];
  const uint64_t code_lo = v_lo & 15u, code_hi = v_hi & 15u;
  const uint64_t off_lo = u_lo - (P[e_lo] - base_lo), off_hi = u_last - (P[e_hi] - base_hi);
  const uint64_t src_only = side ? CIG_I : CIG_D;
  uint64_t a, b, mx, md, heads, head, tail; // the whole entries and chains between the two end entries; the columns of the end entries
  if (link_lo == link_hi) {                 // docs/design/04_25_lift_identity.md
    if (e_lo == e_hi) {
      a = b = mx = md = 0;
      head = off_hi - off_lo + 1u;
      tail = 0;
    } else {
      a = PA[e_hi] - PA[e_lo + 1u], b = PB[e_hi] - PB[e_lo + 1u], mx = PX[e_hi] - PX[e_lo + 1u], md = PD[e_hi] - PD[e_lo + 1u];
      head = (v_lo >> 4) - off_lo;
      tail = off_hi + 1u;
    }
    heads = PH[e_hi + 1u] - PH[e_lo + 1u];
  } else { // the rest of link_lo's chain behind e_lo, the chains of the links between, the chain of link_hi in front of e_hi
    const uint64_t m0 = link_lo + 1u; // m0 <= link_hi <= n_links - 1: the link prefixes have n_links + 1 entries
    a = (PA[end_lo] - PA[e_lo + 1u]) + (LA[link_hi] - LA[m0]) + (PA[e_hi] - PA[f_hi]);
    b = (PB[end_lo] - PB[e_lo + 1u]) + (LB[link_hi] - LB[m0]) + (PB[e_hi] - PB[f_hi]);
    mx = (PX[end_lo] - PX[e_lo + 1u]) + (LX[link_hi] - LX[m0]) + (PX[e_hi] - PX[f_hi]);
    md = (PD[end_lo] - PD[e_lo + 1u]) + (LD[link_hi] - LD[m0]) + (PD[e_hi] - PD[f_hi]);
    const uint64_t code_f = cigar[f_hi] & 15u; // (a chain's own first entry opens a run of its kind)
    heads = (PH[end_lo] - PH[e_lo + 1u]) + (LH[link_hi] - LH[m0]) + (PH[e_hi + 1u] - PH[f_hi + 1u]) +
            (code_f == CIG_I ? 1ull : code_f == CIG_D ? 1ull << 32 : 0);
    head = (v_lo >> 4) - off_lo;
    tail = off_hi + 1u;
  }
  const uint64_t meq = a - mx - md, mi = b - meq - mx;
  const uint32_t i_heads = (uint32_t)heads, d_heads = (uint32_t)(heads >> 32);
  const uint32_t opens = code_lo == src_only ? 1u : 0u; // (a run cut by the range's start counts once)
  const bool both_lo = code_lo == CIG_EQ || code_lo == CIG_X, both_hi = code_hi == CIG_EQ || code_hi == CIG_X;
  // the open stretches between link_lo and link_hi: what lies between the two end chains less the chains between them
  const uint64_t between_src = link_lo == link_hi ? 0 : (side ? LB : LA)[link_hi] - (side ? LB : LA)[link_lo + 1u];
  const uint64_t between_oth = link_lo == link_hi ? 0 : (side ? LA : LB)[link_hi] - (side ? LA : LB)[link_lo + 1u];
  out.src_lo = src_lo;
  out.src_hi = src_hi;
  out.oth_lo = o0_lo + (O[e_lo] - O[f_lo]) + (both_lo ? off_lo : 0);
  out.oth_hi = o0_hi + (O[e_hi] - O[f_hi]) + (both_hi ? off_hi + 1u : 0);
  out.eq = meq + (code_lo == CIG_EQ ? head : 0) + (code_hi == CIG_EQ ? tail : 0);
  out.x = mx + (code_lo == CIG_X ? head : 0) + (code_hi == CIG_X ? tail : 0);
  out.src_gap = (side ? mi : md) + (code_lo == src_only ? head : 0) + (code_hi == src_only ? tail : 0);
  out.oth_gap = side ? md : mi; // (e_lo and e_hi consume the source: a column of the other side alone lies between them)
  out.src_open = link_lo == link_hi ? 0 : s0_hi - s1_lo - between_src;
  out.oth_open = link_lo == link_hi ? 0 : o0_hi - o1_lo - between_oth;
  out.src_gaps = (side ? i_heads : d_heads) + opens;
  out.oth_gaps = side ? d_heads : i_heads;
  out.link_lo = (uint32_t)link_lo;
  out.link_hi = (uint32_t)link_hi;
  out.n_links = (uint32_t)(link_hi - link_lo + 1u);
  stats[g] = out;
}

// the link scan (the size query with tmp = nullptr)
hipError_t lpair_scan(void* tmp, size_t& bytes, const uint64_t* totals, uint64_t* prefixes, uint64_t n_links, hipStream_t stream)
{
  const uint64_t rows = n_links + 1;
  auto adds = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), LpairTotalsOf{ totals, n_links });
  auto out = rocprim::make_zip_iterator(rocprim::make_tuple(prefixes, prefixes + rows, prefixes + 2 * rows, prefixes + 3 * rows, prefixes + 4 * rows));
  return rocprim::exclusive_scan(tmp, bytes, adds, out, LiftStatTuple(0, 0, 0, 0, 0), rows, CigTupleAdd(), stream);
}

int cigar_lift_pairs_run(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains, const nts_lift_link* links,
                         uint64_t n_links, const uint64_t* pair_first, uint64_t n_pairs, const nts_pair_range* ranges, uint64_t n_ranges, nts_pair_stats* stats)
{
  if (const int rc = cig_chains_check(ctx, "nts_cigar_lift_pairs", LIFT_MAX_BASES_LOG2, false, chains, n_chains, n_cigar, [](uint64_t, auto) { return NTS_OK; })) return rc;
  for (uint64_t p = 0; p <= n_pairs; ++p) { // (a loop over pairs: none over links)
    const bool bad = p == 0 ? pair_first[0] != 0 : pair_first[p] < pair_first[p - 1];
    if (bad || (p == n_pairs && pair_first[p] != n_links) || pair_first[p] > n_links)
      return fail(ctx, NTS_EINVAL, "nts_cigar_lift_pairs: pair_first[" + std::to_string(p) + "]: pair_first is not nondecreasing from 0 to n_links");
  }
  // (its own buffers first: while nothing is queued, a request that fails may still return at once)
  NTS_WS(d_links, nts_lift_link*, "lpair_links", std::max<uint64_t>(n_links, 1) * sizeof(nts_lift_link));
  NTS_WS(d_first, uint64_t*, "lpair_first", (n_pairs + 1) * 8);
  NTS_WS(d_owner, uint32_t*, "lpair_owner", std::max<uint64_t>(n_chains, 1) * 4);
  NTS_WS(d_place, LpairPlace*, "lpair_place", std::max<uint64_t>(n_links, 1) * sizeof(LpairPlace));
  NTS_WS(d_totals, uint64_t*, "lpair_totals", 5 * std::max<uint64_t>(n_links, 1) * 8);
  NTS_WS(d_prefixes, uint64_t*, "lpair_prefixes", 5 * (n_links + 1) * 8);
  NTS_WS(d_ranges, nts_pair_range*, "lpair_ranges", std::max<uint64_t>(n_ranges, 1) * sizeof(nts_pair_range));
  NTS_WS(d_stats, nts_pair_stats*, "lpair_stats", std::max<uint64_t>(n_ranges, 1) * sizeof(nts_pair_stats));
  NTS_WS(d_worst, uint32_t*, "lpair_worst", 2 * 4); // the smallest bad link, the smallest bad range
  size_t tmp_l = 0;                                  // the link scan's temporary: a buffer of its own ("ivs_tmp" is the stage's, fetched once inside it)
  HIP_TRY(ctx, lpair_scan(nullptr, tmp_l, d_totals, d_prefixes, n_links, ctx->stream));
  NTS_WS(d_tmp, void*, "lpair_tmp", std::max<size_t>(tmp_l, 16));
  nts_pair_stats* host_stats = n_ranges ? (nts_pair_stats*)malloc(n_ranges * sizeof(nts_pair_stats)) : nullptr; // (the caller's array is written only on success)
  if (n_ranges && !host_stats) return fail(ctx, NTS_ENOMEM, "nts_cigar_lift_pairs: no host memory for the records");
  uint32_t worst[3] = { SCRIPT_OK, SCRIPT_OK, SCRIPT_OK }; // the smallest offending chain, link, range
  CigIndex ix; // columns PA, PB, PX, PD, PH
  hipError_t e_run, e_behind = hipSuccess;
  const uint64_t rows = n_links + 1;
  auto pass_one = [&] { // behind the stage's check, under its timer
    e_behind = hipMemcpyAsync(d_first, pair_first, (n_pairs + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e_behind == hipSuccess && n_links) e_behind = hipMemcpyAsync(d_links, links, n_links * sizeof(nts_lift_link), hipMemcpyHostToDevice, ctx->stream);
    if (e_behind == hipSuccess && n_links) {
      NTS_LAUNCH(k_lpair_claim, IVL_GRID(n_links), (const nts_lift_link*)d_links, n_links, n_chains, d_owner);
      NTS_LAUNCH(k_lpair_twice, IVL_GRID(n_links), (const nts_lift_link*)d_links, n_links, n_chains, d_owner);
      NTS_LAUNCH(k_lpair_links, IVL_GRID(n_links), ix.cigar, n_cigar, ix.chains, n_chains, ix.column(0), ix.column(1), ix.column(2), ix.column(3), ix.column(4),
                 (const nts_lift_link*)d_links, n_links, (const uint64_t*)d_first, n_pairs, (const uint32_t*)d_owner, d_place, d_totals, ix.status);
      e_behind = rocprim::reduce(ix.tmp, ix.tmp_bytes, ix.status, d_worst, SCRIPT_OK, n_links, ScriptMin(), ctx->stream);
    }
    if (e_behind == hipSuccess) e_behind = lpair_scan(d_tmp, tmp_l, d_totals, d_prefixes, n_links, ctx->stream);
  };
  if (const int rc = cig_index_stage<LiftStatOf>(ctx, "lift_pairs_scan", cigar, n_cigar, chains, n_chains, std::max(n_links, n_ranges), &worst[0], ix, e_run,
                                                 pass_one)) {
    free(host_stats);
    return rc;
  }
  if (e_run == hipSuccess) e_run = e_behind;
  if (e_run == hipSuccess && n_ranges) e_run = hipMemcpyAsync(d_ranges, ranges, n_ranges * sizeof(nts_pair_range), hipMemcpyHostToDevice, ctx->stream);
  if (e_run == hipSuccess && n_ranges) { // (no range: nothing more is launched)
    ScopedTimer t(ctx, "lift_pairs_search", true);
    NTS_LAUNCH(k_lpair_ranges, IVL_GRID(n_ranges), ix.cigar, ix.column(0), ix.column(1), ix.column(2), ix.column(3), ix.column(4), (const LpairPlace*)d_place, n_links,
               (const uint64_t*)d_prefixes, (const uint64_t*)(d_prefixes + rows), (const uint64_t*)(d_prefixes + 2 * rows), (const uint64_t*)(d_prefixes + 3 * rows),
               (const uint64_t*)(d_prefixes + 4 * rows), (const uint64_t*)d_first, n_pairs, (const nts_pair_range*)d_ranges, n_ranges, d_stats, ix.status);
    e_run = rocprim::reduce(ix.tmp, ix.tmp_bytes, ix.status, d_worst + 1, SCRIPT_OK, n_ranges, ScriptMin(), ctx->stream);
  }
  if (e_run == hipSuccess) e_run = hipGetLastError();
  if (e_run == hipSuccess && n_links) e_run = hipMemcpyAsync(&worst[1], d_worst, 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e_run == hipSuccess && n_ranges) e_run = hipMemcpyAsync(&worst[2], d_worst + 1, 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e_run == hipSuccess && n_ranges) e_run = hipMemcpyAsync(host_stats, d_stats, n_ranges * sizeof(nts_pair_stats), hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t e_sync = hipStreamSynchronize(ctx->stream); // (whatever happened: the caller's arrays were sources of asynchronous copies)
  const bool good = e_run == hipSuccess && e_sync == hipSuccess && worst[0] == SCRIPT_OK && worst[1] == SCRIPT_OK && worst[2] == SCRIPT_OK;
  if (good && n_ranges) memcpy(stats, host_stats, n_ranges * sizeof(nts_pair_stats));
  free(host_stats);
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  if (worst[0] != SCRIPT_OK)
    return fail(ctx, NTS_EINVAL, "nts_cigar_lift_pairs: the entries of chain " + std::to_string(worst[0]) + " are no CIGAR of its lengths");
  if (worst[1] != SCRIPT_OK) return fail(ctx, NTS_EINVAL, "nts_cigar_lift_pairs: link " + std::to_string(worst[1]) + " is no placement of its chain");
  if (worst[2] != SCRIPT_OK) return fail(ctx, NTS_EINVAL, "nts_cigar_lift_pairs: range " + std::to_string(worst[2]) + " is no range of a pair");
  return NTS_OK;
}

// ---- one liftover chain per PAIR of chains: blocks and their text (nts_cigar_chain_blocks; ntsynt_amd/assess.py chain_table) ----
// docs/design/04_28_block_chain.md.  Input: CIGAR entries, chain records, links and pair_first as for nts_cigar_lift_pairs.  The pair's
// columns are those of its linked chains in link order; a BLOCK is a maximal run of = / X columns with no gap of non-zero width inside
// it, a gap being a D entry (A bases, dt), an I entry (B bases, dq) or the open stretch between two links (both).  Linked entry v is
// entry v - LN[i] of link i's chain, LN the prefix of the links' entry counts: the linked entries in pair order, NV of them.
//   1  cig_index_stage with (A bases, B bases); behind its check k_lpair_claim and k_lpair_twice, k_cchn_links -- one lane per link --
//      validates the link as k_lpair_links does and writes its placement, its pair and its entry count; a minimum reduction names the
//      smallest bad link, ONE exclusive scan over n_links + 1 counts gives LN (timer "chain_blocks_scan").
//   2  k_cchn_cols: one lane per linked entry; a match entry is a HEAD when it is its pair's first linked entry or what lies in front
//      of it in the pair is a gap of non-zero width: a seam's open stretch, else the entry in front of it (across a closed seam, the
//      previous link's last entry).  ONE exclusive scan over the linked entries of (match columns, X columns, A gap bases, B gap bases,
//      heads, last match entry + 1 -- a maximum) follows; k_cchn_heads stores every head at its block index, k_cchn_blocks -- one lane
//      per block -- takes size, dt and dq as prefix differences between two heads, k_cchn_pairs -- one lane per pair -- the record
//      (timer "chain_blocks_emit").
//   3  ONE exclusive scan of the blocks' byte counts, k_cchn_text_firsts, and k_cchn_text: one lane per aligned 4-byte word of the
//      text, as k_cig_text (timer "chain_text").
// No atomic, no launch per pair, chain, link or block, no floating point, no host loop over entries, links or blocks.

static_assert(sizeof(nts_chain_block) == 24 && sizeof(nts_chain_pair) == 64, "the C ABI's layout");

using CchnTuple = rocprim::tuple<uint64_t, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t>; // match, X, A gap, B gap, heads, last match + 1
constexpr uint32_t CCHN_COLUMNS = 6;

struct ChainBasesOf // element e of the stage's scan: what entry e consumes; nothing behind the last entry
{
  using Tuple = CigBases;
  const uint64_t* cigar;
  uint64_t n_cigar;
  __host__ __device__ Tuple operator()(uint64_t e) const { return e < n_cigar ? cig_bases(cigar[e]) : Tuple(0, 0); }
};

struct CchnCountOf // element i of the link scan's input: the entries of link i's chain, 0 for a bad link; nothing behind the last link
{
  const uint64_t* count;
  uint64_t n_links;
  __host__ __device__ uint64_t operator()(uint64_t i) const { return i < n_links ? count[i] : 0; }
};

struct CchnAdd // five sums and a maximum
{
  __host__ __device__ CchnTuple operator()(const CchnTuple& x, const CchnTuple& y) const
  {
    const uint64_t lx = rocprim::get<5>(x), ly = rocprim::get<5>(y);
    return CchnTuple(rocprim::get<0>(x) + rocprim::get<0>(y), rocprim::get<1>(x) + rocprim::get<1>(y), rocprim::get<2>(x) + rocprim::get<2>(y),
                     rocprim::get<3>(x) + rocprim::get<3>(y), rocprim::get<4>(x) + rocprim::get<4>(y), lx > ly ? lx : ly);
  }
};

// the decimal digit of weight 10^j of any v, j <= 19: v = hi 10^9 + lo by the constant 10^9 (a multiplication), hi < 2^35 and lo < 10^9
// are dividends cig_digit is exact for
__device__ __forceinline__ uint32_t cchn_digit(uint64_t v, uint32_t j)
{
  const uint64_t hi = v / 1000000000ull, lo = v - hi * 1000000000ull;
  return j < 9u ? cig_digit(lo, j) : cig_digit(hi, j - 9u);
}

// the bytes of a block's line: "size\n" behind a pair's last block -- the one block without a gap behind it --, else "size\tdt\tdq\n"
__device__ __forceinline__ uint64_t cchn_line_bytes(const nts_chain_block& b)
{
  return (b.dt | b.dq) == 0 ? cig_digits(b.size) + 1u : cig_digits(b.size) + cig_digits(b.dt) + cig_digits(b.dq) + 3u;
}

__global__ __launch_bounds__(256) void k_cchn_links(const nts_cig_chain* __restrict__ chains, uint64_t n_chains, uint64_t n_cigar,
                                                    const nts_lift_link* __restrict__ links, uint64_t n_links, const uint64_t* __restrict__ pair_first,
                                                    uint64_t n_pairs, const uint32_t* __restrict__ owner, LpairPlace* __restrict__ place,
                                                    uint32_t* __restrict__ pair_of, uint64_t* __restrict__ count, uint32_t* __restrict__ status)
{
  const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (g >= n_links) return;
  const nts_lift_link lk = links[g];
  nts_cig_chain ch;
  // (a chain without entries may not be linked; behind this first + n_cig <= n_cigar and n_cig >= 1)
  bool ok = lk.reserved == 0 && cig_chain_of(chains, n_chains, lk.chain, 0u, ch) && !cig_chain_beyond(ch, n_cigar) && ch.n_cig != 0;
  ok = ok && owner[lk.chain] != LPAIR_TWICE; // (lk.chain < n_chains)
  ok = ok && lk.a0 < LPAIR_MAX_BASE && lk.b0 < LPAIR_MAX_BASE && ch.len_a < LPAIR_MAX_BASE - lk.a0 && ch.len_b < LPAIR_MAX_BASE - lk.b0;
  // its pair: the last with pair_first <= g (pair_first[0] = 0 <= g < n_links = pair_first[n_pairs]: n_pairs >= 1 here)
  const uint64_t p = cig_last_at_or_before(n_pairs, g, [pair_first](uint64_t i) { return pair_first[i]; });
  if (ok && g > pair_first[p]) { // the link in front of it in its pair; one that is bad itself is named instead
    const nts_lift_link pv = links[g - 1u];
    nts_cig_chain pc;
    if (cig_chain_of(chains, n_chains, pv.chain, 0u, pc) && pv.a0 < LPAIR_MAX_BASE && pv.b0 < LPAIR_MAX_BASE && pc.len_a < LPAIR_MAX_BASE - pv.a0 &&
        pc.len_b < LPAIR_MAX_BASE - pv.b0)
      ok = lk.a0 >= pv.a0 + pc.len_a && lk.b0 >= pv.b0 + pc.len_b;
  }
  if (ok) place[g] = { ch.first, ch.n_cig, lk.a0, lk.a0 + ch.len_a, lk.b0, lk.b0 + ch.len_b };
  else place[g] = { 0, 0, lk.a0, lk.a0, lk.b0, lk.b0 };
  pair_of[g] = (uint32_t)p;
  count[g] = ok ? ch.n_cig : 0;
  status[g] = ok ? SCRIPT_OK : (uint32_t)g;
}

// lane v <= cap: what linked entry v adds to the six columns `in` (rows words each), zeros behind the last linked entry
__global__ __launch_bounds__(256) void k_cchn_cols(const uint64_t* __restrict__ cigar, uint64_t n_cigar, const LpairPlace* __restrict__ place,
                                                   const uint32_t* __restrict__ pair_of, const uint64_t* __restrict__ LN, uint64_t n_links,
                                                   const uint64_t* __restrict__ pair_first, uint64_t n_pairs, uint64_t cap, uint64_t* __restrict__ in,
                                                   uint32_t* __restrict__ link_of)
{
  const uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x, rows = cap + 1u;
  if (v > cap) return;
  uint64_t m = 0, x = 0, ga = 0, gb = 0, head = 0, last = 0;
  const uint64_t nv = LN[n_links] < cap ? LN[n_links] : cap; // (good links name different chains: their entries number cap at the most)
  if (v < nv) {
    // its link: the last with LN <= v (LN[0] = 0 <= v < LN[n_links]); LN[i + 1] > v, so link i has entries: a good link
    const uint64_t i = cig_last_at_or_before(n_links, v, [LN](uint64_t k) { return LN[k]; });
    const LpairPlace pl = place[i];
    uint64_t p = pair_of[i];
    if (p >= n_pairs) p = n_pairs - 1u; // (k_cchn_links stored p < n_pairs)
    uint64_t l0 = pair_first[p];
    if (l0 > i) l0 = i;
    uint64_t k = v - LN[i];
    if (k >= pl.n_cig) k = pl.n_cig - 1u; // (LN[i + 1] - LN[i] = n_cig > k)
    uint64_t e = pl.first + k;
    if (e >= n_cigar) e = n_cigar - 1u; // (k_cchn_links: first + n_cig <= n_cigar)
    const uint64_t val = cigar[e], code = val & 15u, len = val >> 4;
    const bool match = code == CIG_EQ || code == CIG_X;
    const bool opens_link = k == 0, opens_pair = v == LN[l0];
    bool gap_in_front = false;
    if (opens_link && !opens_pair) { // a seam: LN[i] > LN[l0] gives i > l0, link i - 1 lies in the same pair
      const LpairPlace pv = place[i - 1u];
      const uint64_t sa = pl.a0 - pv.a1, sb = pl.b0 - pv.b1;
      ga = sa;
      gb = sb;
      if ((sa | sb) != 0 || pv.n_cig == 0) {
        gap_in_front = true;
      } else {
        const uint64_t pe = pv.first + pv.n_cig - 1u; // the previous link's last entry (pe < n_cigar: k_cchn_links)
        const uint64_t pc = pe < n_cigar ? cigar[pe] & 15u : 0;
        gap_in_front = !(pc == CIG_EQ || pc == CIG_X);
      }
    } else if (!opens_link) {
      const uint64_t pc = cigar[e ? e - 1u : 0] & 15u; // (e > first >= 0)
      gap_in_front = !(pc == CIG_EQ || pc == CIG_X);
    }
    if (match) {
      m = len;
      x = code == CIG_X ? len : 0;
      head = opens_pair || gap_in_front ? 1u : 0u;
      last = v + 1u;
    } else {
      ga += code == CIG_D ? len : 0;
      gb += code == CIG_I ? len : 0;
    }
    link_of[v] = (uint32_t)i;
  }
  in[v] = m;
  in[rows + v] = x;
  in[2u * rows + v] = ga;
  in[3u * rows + v] = gb;
  in[4u * rows + v] = head;
  in[5u * rows + v] = last;
}

// every head stores its linked entry at its block index
__global__ __launch_bounds__(256) void k_cchn_heads(const uint64_t* __restrict__ in_head, const uint64_t* __restrict__ PH, uint64_t cap,
                                                    uint32_t* __restrict__ head_at)
{
  const uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (v >= cap || in_head[v] == 0) return;
  const uint64_t j = PH[v];
  if (j < cap) head_at[j] = (uint32_t)v; // (heads in front of v: fewer than cap)
}

// lane j <= cap: block j's size and the gaps behind it, and the bytes of its line; 0 bytes behind the last block
__global__ __launch_bounds__(256) void k_cchn_blocks(const uint32_t* __restrict__ head_at, const uint32_t* __restrict__ link_of,
                                                     const uint32_t* __restrict__ pair_of, const uint64_t* __restrict__ LN, uint64_t n_links,
                                                     const uint64_t* __restrict__ pair_first, uint64_t n_pairs, const uint64_t* __restrict__ pre, uint64_t cap,
                                                     nts_chain_block* __restrict__ blocks, uint64_t* __restrict__ bytes)
{
  const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x, rows = cap + 1u;
  if (j > cap) return;
  const uint64_t* __restrict__ PM = pre;
  const uint64_t* __restrict__ PGA = pre + 2u * rows;
  const uint64_t* __restrict__ PGB = pre + 3u * rows;
  const uint64_t nb = pre[4u * rows + cap] < cap ? pre[4u * rows + cap] : cap; // the heads of all linked entries
  if (j >= nb) {
    bytes[j] = 0;
    return;
  }
  uint64_t v = head_at[j];
  if (v >= cap) v = cap - 1u; // (k_cchn_heads stored v < cap)
  uint64_t i = link_of[v];
  if (i >= n_links) i = n_links - 1u;
  uint64_t p = pair_of[i];
  if (p >= n_pairs) p = n_pairs - 1u;
  uint64_t l1 = pair_first[p + 1u];
  if (l1 > n_links) l1 = n_links;
  uint64_t v_end = LN[l1]; // behind the pair's last linked entry
  if (v_end > cap) v_end = cap;
  uint64_t next = v_end;
  bool is_last = true;
  if (j + 1u < nb) {
    const uint64_t nx = head_at[j + 1u];
    if (nx < v_end) next = nx, is_last = false;
  }
  if (next < v) next = v; // (heads ascend with their index)
  nts_chain_block b = { PM[next] - PM[v], 0, 0 };
  if (!is_last) { // the gaps of the linked entries v + 1 .. next, the seam in front of `next` included (next + 1 <= cap)
    b.dt = PGA[next + 1u] - PGA[v + 1u];
    b.dq = PGB[next + 1u] - PGB[v + 1u];
  }
  blocks[j] = b;
  bytes[j] = cchn_line_bytes(b);
}

// lane p < n_pairs: the record of pair p's liftover chain, all 0 for a pair without a match column
__global__ __launch_bounds__(256) void k_cchn_pairs(const LpairPlace* __restrict__ place, const uint32_t* __restrict__ head_at,
                                                    const uint32_t* __restrict__ link_of, const uint64_t* __restrict__ LN, uint64_t n_links,
                                                    const uint64_t* __restrict__ pair_first, uint64_t n_pairs, const uint64_t* __restrict__ pre, uint64_t cap,
                                                    const uint64_t* __restrict__ PA, const uint64_t* __restrict__ PB, uint64_t n_cigar,
                                                    nts_chain_pair* __restrict__ pairs)
{
  const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x, rows = cap + 1u;
  if (p >= n_pairs) return;
  uint64_t l0 = pair_first[p], l1 = pair_first[p + 1u];
  if (l1 > n_links) l1 = n_links; // (the host refused this before the launch: a lane still reads nothing outside the link prefixes)
  if (l0 > l1) l0 = l1;
  uint64_t v0 = LN[l0], v1 = LN[l1];
  if (v1 > cap) v1 = cap;
  if (v0 > v1) v0 = v1;
  const uint64_t* __restrict__ PM = pre;
  const uint64_t* __restrict__ PX = pre + rows;
  const uint64_t* __restrict__ PH = pre + 4u * rows;
  const uint64_t* __restrict__ PL = pre + 5u * rows;
  const uint64_t fb = PH[v0], nb = PH[v1] - fb;
  nts_chain_pair out = {};
  if (nb == 0 || fb >= cap) {
    pairs[p] = out;
    return;
  }
  uint64_t h = head_at[fb], t = PL[v1] - 1u; // the pair's first and last match entry (PL[v1] >= h + 1: a maximum over all entries in front of v1)
  if (h >= cap) h = cap - 1u;
  if (t >= cap || t < h) t = h;
  uint64_t ih = link_of[h], it = link_of[t];
  if (ih >= n_links) ih = n_links - 1u;
  if (it >= n_links) it = n_links - 1u;
  const LpairPlace ph = place[ih], pt = place[it];
  uint64_t eh = ph.first + (h - LN[ih]), et = pt.first + (t - LN[it]);
  if (eh >= n_cigar) eh = n_cigar - 1u; // (first <= e < first + n_cig <= n_cigar for the entries of a good link)
  if (et >= n_cigar) et = n_cigar - 1u;
  const uint64_t fh = ph.first <= eh ? ph.first : eh, ft = pt.first <= et ? pt.first : et;
  out.a0 = ph.a0 + (PA[eh] - PA[fh]);
  out.b0 = ph.b0 + (PB[eh] - PB[fh]);
  out.a1 = pt.a0 + (PA[et + 1u] - PA[ft]);
  out.b1 = pt.b0 + (PB[et + 1u] - PB[ft]);
  out.x = PX[v1] - PX[h];
  out.eq = (PM[v1] - PM[h]) - out.x;
  out.first_block = fb;
  out.n_blocks = (uint32_t)nb;
  pairs[p] = out;
}

// lane p <= n_pairs: where pair p's lines begin, the text's length for p = n_pairs
__global__ __launch_bounds__(256) void k_cchn_text_firsts(const uint64_t* __restrict__ LN, uint64_t n_links, const uint64_t* __restrict__ pair_first,
                                                          uint64_t n_pairs, const uint64_t* __restrict__ PH, const uint64_t* __restrict__ TB, uint64_t cap,
                                                          uint64_t* __restrict__ text_first)
{
  const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (p > n_pairs) return;
  uint64_t l = pair_first[p];
  if (l > n_links) l = n_links;
  uint64_t v = LN[l];
  if (v > cap) v = cap;
  uint64_t fb = PH[v];
  if (fb > cap) fb = cap;
  text_first[p] = TB[fb];
}

// one lane per aligned 4-byte word of the text: the block of the word's first byte by a search over the byte prefix, then the at most
// three further lines a word touches (a line has at least 2 bytes)
__global__ __launch_bounds__(256) void k_cchn_text(const nts_chain_block* __restrict__ blocks, uint64_t n_blocks, const uint64_t* __restrict__ TB,
                                                   uint32_t* __restrict__ out, uint64_t n_words)
{
  const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (w >= n_words || n_blocks == 0) return;
  const uint64_t total = TB[n_blocks], o = 4u * w;
  uint64_t j = cig_last_at_or_before(n_blocks, o, [TB](uint64_t i) { return TB[i]; }); // (TB[0] = 0 <= o)
  uint64_t p0 = TB[j], p1 = TB[j + 1u]; // (j < n_blocks)
  nts_chain_block b = blocks[j];
  uint32_t word = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    const uint64_t at = o + k;
    if (at >= total) break; // (the padding of the last word stays 0)
    while (at >= p1 && j + 1u < n_blocks) {
      ++j;
      p0 = p1;
      p1 = TB[j + 1u];
      b = blocks[j];
    }
    const bool is_last = (b.dt | b.dq) == 0;
    uint64_t off = at - p0, number = b.size;
    uint32_t end = is_last ? '\n' : '\t';
    uint32_t digits = cig_digits(number);
    if (!is_last && off > digits) { // behind "size\t"
      off -= digits + 1u;
      number = b.dt;
      digits = cig_digits(number);
      if (off > digits) { // behind "dt\t"
        off -= digits + 1u;
        number = b.dq;
        digits = cig_digits(number);
        end = '\n';
      }
    }
    const uint32_t byte = off < digits ? '0' + cchn_digit(number, digits - 1u - (uint32_t)off) : end;
    word |= byte << (8u * k);
  }
  out[w] = word;
}

// the link scan, the scan over the linked entries and the scan of the blocks' bytes (the size queries with tmp = nullptr)
hipError_t cchn_link_scan(void* tmp, size_t& bytes, const uint64_t* count, uint64_t* LN, uint64_t n_links, hipStream_t stream)
{
  auto adds = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), CchnCountOf{ count, n_links });
  return rocprim::exclusive_scan(tmp, bytes, adds, LN, (uint64_t)0, n_links + 1, rocprim::plus<uint64_t>(), stream);
}

hipError_t cchn_entry_scan(void* tmp, size_t& bytes, const uint64_t* in, uint64_t* pre, uint64_t cap, hipStream_t stream)
{
  const uint64_t rows = cap + 1;
  auto adds = rocprim::make_zip_iterator(rocprim::make_tuple(in, in + rows, in + 2 * rows, in + 3 * rows, in + 4 * rows, in + 5 * rows));
  auto out = rocprim::make_zip_iterator(rocprim::make_tuple(pre, pre + rows, pre + 2 * rows, pre + 3 * rows, pre + 4 * rows, pre + 5 * rows));
  return rocprim::exclusive_scan(tmp, bytes, adds, out, CchnTuple(0, 0, 0, 0, 0, 0), rows, CchnAdd(), stream);
}

hipError_t cchn_byte_scan(void* tmp, size_t& bytes, const uint64_t* line_bytes, uint64_t* TB, uint64_t cap, hipStream_t stream)
{
  return rocprim::exclusive_scan(tmp, bytes, line_bytes, TB, (uint64_t)0, cap + 1, rocprim::plus<uint64_t>(), stream);
}

int cigar_chain_blocks_run(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains, const nts_lift_link* links,
                           uint64_t n_links, const uint64_t* pair_first, uint64_t n_pairs, nts_chain_pair* pairs, nts_chain_block** blocks, uint64_t* n_blocks,
                           uint8_t** text, uint64_t* text_first)
{
  const bool with_text = text != nullptr;
  uint64_t entries = 0; // the entries of all chains: good links name different chains, so they link at most that many
  auto count = [&](uint64_t c, auto) {
    entries += chains[c].n_cig; // (n_cig <= n_cigar < 2^32 and fewer than 2^32 chains: no wrap)
    return NTS_OK;
  };
  if (const int rc = cig_chains_check(ctx, "nts_cigar_chain_blocks", LIFT_MAX_BASES_LOG2, false, chains, n_chains, n_cigar, count)) return rc;
  if (entries > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_cigar_chain_blocks: the chains hold 2^32 entries or more");
  for (uint64_t p = 0; p <= n_pairs; ++p) { // (a loop over pairs: none over links)
    const bool bad = p == 0 ? pair_first[0] != 0 : pair_first[p] < pair_first[p - 1];
    if (bad || (p == n_pairs && pair_first[p] != n_links) || pair_first[p] > n_links)
      return fail(ctx, NTS_EINVAL, "nts_cigar_chain_blocks: pair_first[" + std::to_string(p) + "]: pair_first is not nondecreasing from 0 to n_links");
  }
  const uint64_t cap = std::max<uint64_t>(entries, 1), rows = cap + 1;
  // (its own buffers first: while nothing is queued, a request that fails may still return at once)
  NTS_WS(d_links, nts_lift_link*, "cchn_links", std::max<uint64_t>(n_links, 1) * sizeof(nts_lift_link));
  NTS_WS(d_first, uint64_t*, "cchn_first", (n_pairs + 1) * 8);
  NTS_WS(d_owner, uint32_t*, "cchn_owner", std::max<uint64_t>(n_chains, 1) * 4);
  NTS_WS(d_place, LpairPlace*, "cchn_place", std::max<uint64_t>(n_links, 1) * sizeof(LpairPlace));
  NTS_WS(d_pair_of, uint32_t*, "cchn_pair_of", std::max<uint64_t>(n_links, 1) * 4);
  NTS_WS(d_count, uint64_t*, "cchn_count", std::max<uint64_t>(n_links, 1) * 8);
  NTS_WS(d_ln, uint64_t*, "cchn_ln", (n_links + 1) * 8);
  NTS_WS(d_in, uint64_t*, "cchn_in", CCHN_COLUMNS * rows * 8);
  NTS_WS(d_pre, uint64_t*, "cchn_pre", CCHN_COLUMNS * rows * 8);
  NTS_WS(d_link_of, uint32_t*, "cchn_link_of", cap * 4);
  NTS_WS(d_head_at, uint32_t*, "cchn_head_at", cap * 4);
  NTS_WS(d_blocks, nts_chain_block*, "cchn_blocks", cap * sizeof(nts_chain_block));
  NTS_WS(d_bytes, uint64_t*, "cchn_bytes", rows * 8);
  NTS_WS(d_tb, uint64_t*, "cchn_tb", rows * 8);
  NTS_WS(d_pairs, nts_chain_pair*, "cchn_pairs", std::max<uint64_t>(n_pairs, 1) * sizeof(nts_chain_pair));
  NTS_WS(d_tfirst, uint64_t*, "cchn_tfirst", (n_pairs + 1) * 8);
  NTS_WS(d_worst, uint32_t*, "cchn_worst", 2 * 4);
  size_t tmp_l = 0, tmp_v = 0, tmp_b = 0; // the three scans' temporary: a buffer of its own ("ivs_tmp" is the stage's, fetched once inside it)
  HIP_TRY(ctx, cchn_link_scan(nullptr, tmp_l, d_count, d_ln, n_links, ctx->stream));
  HIP_TRY(ctx, cchn_entry_scan(nullptr, tmp_v, d_in, d_pre, cap, ctx->stream));
  HIP_TRY(ctx, cchn_byte_scan(nullptr, tmp_b, d_bytes, d_tb, cap, ctx->stream));
  NTS_WS(d_tmp, void*, "cchn_tmp", std::max<size_t>(std::max(tmp_l, std::max(tmp_v, tmp_b)), 16));
  std::vector<nts_chain_pair> host_pairs(n_pairs); // (the caller's arrays are written only when the call succeeds)
  std::vector<uint64_t> host_first(n_pairs + 1, 0);
  uint32_t worst[2] = { SCRIPT_OK, SCRIPT_OK }; // the smallest offending chain, link
  uint64_t num[2] = { 0, 0 };                   // blocks, text bytes
  CigIndex ix; // columns PA, PB
  hipError_t e_run, e_behind = hipSuccess;
  auto pass_one = [&] { // behind the stage's check, under its timer
    if (n_links == 0) return;
    e_behind = hipMemcpyAsync(d_first, pair_first, (n_pairs + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e_behind == hipSuccess) e_behind = hipMemcpyAsync(d_links, links, n_links * sizeof(nts_lift_link), hipMemcpyHostToDevice, ctx->stream);
    if (e_behind != hipSuccess) return;
    NTS_LAUNCH(k_lpair_claim, IVL_GRID(n_links), (const nts_lift_link*)d_links, n_links, n_chains, d_owner);
    NTS_LAUNCH(k_lpair_twice, IVL_GRID(n_links), (const nts_lift_link*)d_links, n_links, n_chains, d_owner);
    NTS_LAUNCH(k_cchn_links, IVL_GRID(n_links), ix.chains, n_chains, n_cigar, (const nts_lift_link*)d_links, n_links, (const uint64_t*)d_first, n_pairs,
               (const uint32_t*)d_owner, d_place, d_pair_of, d_count, ix.status);
    e_behind = rocprim::reduce(ix.tmp, ix.tmp_bytes, ix.status, d_worst, SCRIPT_OK, n_links, ScriptMin(), ctx->stream);
    if (e_behind == hipSuccess) e_behind = cchn_link_scan(d_tmp, tmp_l, d_count, d_ln, n_links, ctx->stream);
  };
  if (const int rc = cig_index_stage<ChainBasesOf>(ctx, "chain_blocks_scan", cigar, n_cigar, chains, n_chains, n_links, &worst[0], ix, e_run, pass_one)) return rc;
  if (e_run == hipSuccess) e_run = e_behind;
  if (e_run == hipSuccess && n_links) { // (no link: nothing more is launched)
    ScopedTimer t(ctx, "chain_blocks_emit", true);
    NTS_LAUNCH(k_cchn_cols, IVL_GRID(rows), ix.cigar, n_cigar, (const LpairPlace*)d_place, (const uint32_t*)d_pair_of, (const uint64_t*)d_ln, n_links,
               (const uint64_t*)d_first, n_pairs, cap, d_in, d_link_of);
    e_run = cchn_entry_scan(d_tmp, tmp_v, d_in, d_pre, cap, ctx->stream);
    if (e_run == hipSuccess) {
      NTS_LAUNCH(k_cchn_heads, IVL_GRID(cap), (const uint64_t*)(d_in + 4 * rows), (const uint64_t*)(d_pre + 4 * rows), cap, d_head_at);
      NTS_LAUNCH(k_cchn_blocks, IVL_GRID(rows), (const uint32_t*)d_head_at, (const uint32_t*)d_link_of, (const uint32_t*)d_pair_of, (const uint64_t*)d_ln, n_links,
                 (const uint64_t*)d_first, n_pairs, (const uint64_t*)d_pre, cap, d_blocks, d_bytes);
      if (n_pairs)
        NTS_LAUNCH(k_cchn_pairs, IVL_GRID(n_pairs), (const LpairPlace*)d_place, (const uint32_t*)d_head_at, (const uint32_t*)d_link_of, (const uint64_t*)d_ln,
                   n_links, (const uint64_t*)d_first, n_pairs, (const uint64_t*)d_pre, cap, ix.column(0), ix.column(1), n_cigar, d_pairs);
    }
  }
  if (e_run == hipSuccess && n_links && with_text) {
    ScopedTimer t(ctx, "chain_text", true);
    e_run = cchn_byte_scan(d_tmp, tmp_b, d_bytes, d_tb, cap, ctx->stream);
    if (e_run == hipSuccess)
      NTS_LAUNCH(k_cchn_text_firsts, IVL_GRID(n_pairs + 1), (const uint64_t*)d_ln, n_links, (const uint64_t*)d_first, n_pairs, (const uint64_t*)(d_pre + 4 * rows),
                 (const uint64_t*)d_tb, cap, d_tfirst);
  }
  if (e_run == hipSuccess) e_run = hipGetLastError();
  if (e_run == hipSuccess && n_links) e_run = hipMemcpyAsync(&worst[1], d_worst, 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e_run == hipSuccess && n_links) e_run = hipMemcpyAsync(&num[0], d_pre + 4 * rows + cap, 8, hipMemcpyDeviceToHost, ctx->stream);
  if (e_run == hipSuccess && n_links && with_text) e_run = hipMemcpyAsync(&num[1], d_tb + cap, 8, hipMemcpyDeviceToHost, ctx->stream);
  if (e_run == hipSuccess && n_links && n_pairs)
    e_run = hipMemcpyAsync(host_pairs.data(), d_pairs, n_pairs * sizeof(nts_chain_pair), hipMemcpyDeviceToHost, ctx->stream);
  if (e_run == hipSuccess && n_links && with_text) e_run = hipMemcpyAsync(host_first.data(), d_tfirst, (n_pairs + 1) * 8, hipMemcpyDeviceToHost, ctx->stream);
  hipError_t e_sync = hipStreamSynchronize(ctx->stream); // (whatever happened: the caller's arrays were sources of asynchronous copies)
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  if (worst[0] != SCRIPT_OK)
    return fail(ctx, NTS_EINVAL, "nts_cigar_chain_blocks: the entries of chain " + std::to_string(worst[0]) + " are no CIGAR of its lengths");
  if (worst[1] != SCRIPT_OK) return fail(ctx, NTS_EINVAL, "nts_cigar_chain_blocks: link " + std::to_string(worst[1]) + " is no placement of its chain");
  const uint64_t nb = num[0], text_bytes = num[1];
  if (nb > 0xFFFFFFFFull || nb > cap) return fail(ctx, NTS_ERANGE, "nts_cigar_chain_blocks: 2^32 blocks or more");
  if (text_bytes > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_cigar_chain_blocks: a text of 2^32 bytes or more");
  nts_chain_block* host_blocks = nullptr;
  uint8_t* host_text = nullptr;
  if (nb) { // (the stream is idle: the text's buffer is fetched before its kernel is queued)
    const uint64_t words = (text_bytes + 3) / 4; // (the device buffer is padded to whole words)
    uint32_t* d_text = nullptr;
    if (with_text) {
      d_text = (uint32_t*)ws_get(ctx, "cchn_text", std::max<uint64_t>(words, 1) * 4);
      if (!d_text) return NTS_ENOMEM;
    }
    host_blocks = (nts_chain_block*)malloc(nb * sizeof(nts_chain_block));
    if (with_text) host_text = (uint8_t*)malloc(std::max<uint64_t>(text_bytes, 1));
    if (!host_blocks || (with_text && !host_text)) {
      free(host_blocks);
      free(host_text);
      return fail(ctx, NTS_ENOMEM, "nts_cigar_chain_blocks: no host memory for the blocks");
    }
    if (with_text) {
      ScopedTimer t(ctx, "chain_text", true);
      NTS_LAUNCH(k_cchn_text, IVL_GRID(words), (const nts_chain_block*)d_blocks, nb, (const uint64_t*)d_tb, d_text, words);
    }
    e_run = hipGetLastError();
    if (e_run == hipSuccess) e_run = hipMemcpyAsync(host_blocks, d_blocks, nb * sizeof(nts_chain_block), hipMemcpyDeviceToHost, ctx->stream);
    if (e_run == hipSuccess && with_text && text_bytes) e_run = hipMemcpyAsync(host_text, d_text, text_bytes, hipMemcpyDeviceToHost, ctx->stream);
    e_sync = hipStreamSynchronize(ctx->stream);
    if (e_run != hipSuccess || e_sync != hipSuccess) {
      free(host_blocks);
      free(host_text);
    }
    HIP_TRY(ctx, e_run);
    HIP_TRY(ctx, e_sync);
  }
  if (n_pairs) memcpy(pairs, host_pairs.data(), n_pairs * sizeof(nts_chain_pair)); // (zeros where nothing was linked)
  *blocks = host_blocks;
  *n_blocks = nb;
  if (with_text) {
    *text = host_text;
    memcpy(text_first, host_first.data(), (n_pairs + 1) * 8);
  }
  return NTS_OK;
}

// ---- the aligned rows of the chains' CIGARs: the sequence lines of a MAF block (nts_cigar_rows; ntsynt_amd/assess.py maf_table) ----
// docs/design/04_29_block_maf.md.  Input: entries, chain records and spans as for nts_cigar_text with spans, the chains tiling the entries.
// A COLUMN is one unit of an entry's length; chain c has eq + x + ins + del of them and two ROWS of that many bytes: row A the target
// base of the column (`-` for I), row B the query base as read (`-` for D); upper case ACGT, N for a code that is no base.
//   1  cig_index_stage with (A bases, B bases, columns): three columns; behind its check, k_cig_rows_firsts reads the column prefix at
//      every chain's first entry (timer "cigar_rows_scan").  The chains tile the entries (host check), so a chain's rows are one byte
//      range of either buffer, the same range in both.
//   2  k_cig_rows: one lane per aligned 4-byte word of the rows; ONE upper-bound binary search over the column prefix finds the entry
//      of the word's first column and serves both rows; the lane walks on over the at most three further entries a word touches,
//      composes four bytes per row in two registers and stores two dwords (timer "cigar_rows_emit").  An entry finds its chain by a
//      search over the chains' first entries and a base is one code load at the chain's base address plus the A or B prefix difference.
// No atomic, no launch per chain or entry, no floating point, no runtime division, no host loop over entries.

using CigRowsTuple = rocprim::tuple<uint64_t, uint64_t, uint64_t>; // A bases, B bases, columns

template <bool PADDED_> // (true: nts_cigar_rows_padded, where an entry of code 6 has columns and consumes nothing)
struct CigRowsOf // element e of the scan's input: what entry e consumes and how many columns it has; nothing behind the last entry
{
  using Tuple = CigRowsTuple;
  static constexpr bool PADDED = PADDED_;
  const uint64_t* cigar;
  uint64_t n_cigar;
  __device__ Tuple operator()(uint64_t e) const
  {
    if (e >= n_cigar) return Tuple(0, 0, 0);
    const uint64_t v = cigar[e], code = v & 15u;
    const CigBases ab = cig_bases(v);
    const bool known = code == CIG_EQ || code == CIG_X || code == CIG_I || code == CIG_D || (PADDED && code == CIG_P);
    return Tuple(rocprim::get<0>(ab), rocprim::get<1>(ab), known ? v >> 4 : 0); // (columns <= A bases + B bases: no wrap where those have none)
  }
};

// lane c <= n_chains: where chain c's rows begin, the rows' length for c = n_chains
__global__ __launch_bounds__(256) void k_cig_rows_firsts(const nts_cig_chain* __restrict__ chains, uint64_t n_chains, uint64_t n_cigar,
                                                         const uint64_t* __restrict__ PC, uint64_t* __restrict__ row_first)
{
  const uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (c > n_chains) return;
  uint64_t f = c < n_chains ? chains[c].first : n_cigar;
  if (f > n_cigar) f = n_cigar; // (the host refused this before the launch: a lane still reads nothing outside the prefixes)
  row_first[c] = PC[f];
}

// the letter of the base idx of one side of a chain: 'N' for a code that is no base, complemented or not; '?' -- never seen in a row --
// instead of a load outside the chain or the code array (the chain check and the host's span checks leave none)
__device__ __forceinline__ uint32_t cig_rows_base(const uint8_t* __restrict__ code, uint64_t size, uint64_t at, uint64_t idx, uint64_t len, bool backwards)
{
  if (idx >= len || (backwards ? idx > at : idx >= size - at)) return '?';
  const uint64_t where = backwards ? at - idx : at + idx;
  if (where < PAD || where >= size - PAD) return '?';
  uint32_t c = code[where];
  if (c >= nts::CODE_INVALID) return 'N';
  if (backwards) c = 3u - c;
  return (0x54474341u >> (8u * c)) & 255u; // "ACGT"
}

template <bool PADDED> // (true: a column of an entry of code 6 is `-` in both rows)
__global__ __launch_bounds__(256) void k_cig_rows(const uint64_t* __restrict__ cigar, uint64_t n_cigar, const CigTextChain* __restrict__ chains,
                                                  uint64_t n_chains, const uint64_t* __restrict__ PA, const uint64_t* __restrict__ PB,
                                                  const uint64_t* __restrict__ PC, const uint8_t* __restrict__ code_a, uint64_t size_a,
                                                  const uint8_t* __restrict__ code_b, uint64_t size_b, uint32_t* __restrict__ out_a,
                                                  uint32_t* __restrict__ out_b, uint64_t n_words)
{
  const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (w >= n_words || n_cigar == 0 || n_chains == 0) return;
  const uint64_t total = PC[n_cigar], o = 4u * w;
  uint64_t e = cig_last_at_or_before(n_cigar, o, [PC](uint64_t i) { return PC[i]; }); // the entry of the word's first column (PC[0] = 0 <= o)
  uint64_t p0 = PC[e], p1 = PC[e + 1u]; // (e < n_cigar)
  uint64_t chain_of = ~0ull; // the entry whose chain `ch` is, and where that entry's bases begin inside the chain
  CigTextChain ch = {};
  uint64_t in_a = 0, in_b = 0;
  uint32_t code = 0;
  uint32_t word_a = 0, word_b = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    const uint64_t at = o + k;
    if (at >= total) break;                // (the padding of the last word stays 0)
    while (at >= p1 && e + 1u < n_cigar) { // the next entry: an entry has at least 1 column, so at most three steps per word
      ++e;
      p0 = p1;
      p1 = PC[e + 1u];
    }
    if (chain_of != e) { // the last chain with first <= e (chains[0].first = 0; empty chains in front of it share its first)
      ch = chains[cig_last_at_or_before(n_chains, e, [chains](uint64_t c) { return chains[c].first; })];
      chain_of = e;
      const uint64_t f = ch.first <= e ? ch.first : e;
      in_a = PA[e] - PA[f];
      in_b = PB[e] - PB[f];
      code = (uint32_t)(cigar[e] & 15u);
    }
    const uint64_t off = at - p0;
    const bool pad = PADDED && code == CIG_P;
    const uint32_t byte_a = code == CIG_I || pad ? (uint32_t)'-' : cig_rows_base(code_a, size_a, ch.at_a, in_a + off, ch.len_a, false);
    const uint32_t byte_b = code == CIG_D || pad ? (uint32_t)'-' : cig_rows_base(code_b, size_b, ch.at_b, in_b + off, ch.len_b, (ch.flags & NTS_CIG_B_BACKWARDS) != 0);
    word_a |= byte_a << (8u * k);
    word_b |= byte_b << (8u * k);
  }
  out_a[w] = word_a;
  out_b[w] = word_b;
}

// chain c's span, behind the checks of its record: nts_cigar_text's rules; what nts_cigar_rows and nts_cigar_var_bases refuse alike
template <class Who>
int cig_rows_place(nts_ctx* ctx, const nts_cig_chain& ch, const nts_cig_span& sp, const nts_genome* a, const nts_genome* b, Who who, CigTextChain& placed)
{
  if (sp.flags & ~NTS_CIG_B_BACKWARDS) return fail(ctx, NTS_EINVAL, who() + " has unknown flag bits");
  if (sp.rec_a >= a->n_rec || sp.rec_b >= b->n_rec) return fail(ctx, NTS_EINVAL, who() + " names a record outside its genome");
  const uint64_t rl_a = a->rec_len[sp.rec_a], rl_b = b->rec_len[sp.rec_b];
  const bool backwards = (sp.flags & NTS_CIG_B_BACKWARDS) != 0;
  bool inside = sp.pos_a <= rl_a && ch.len_a <= rl_a - sp.pos_a;
  if (ch.len_b == 0) inside = inside && sp.pos_b <= rl_b;
  else if (backwards) inside = inside && sp.pos_b < rl_b && ch.len_b <= sp.pos_b + 1u;
  else inside = inside && sp.pos_b <= rl_b && ch.len_b <= rl_b - sp.pos_b;
  if (!inside) return fail(ctx, NTS_EINVAL, who() + ": its span lies outside its record");
  placed = { ch.first, PAD + a->rec_off[sp.rec_a] + sp.pos_a, PAD + b->rec_off[sp.rec_b] + sp.pos_b, ch.len_a, ch.len_b, sp.flags, 0u };
  return NTS_OK;
}

template <bool PADDED>
int cigar_rows_run(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains, const nts_genome* a,
                   const nts_genome* b, const nts_cig_span* spans, uint8_t** row_a, uint8_t** row_b, uint64_t* row_first)
{
  const char* const name = PADDED ? "nts_cigar_rows_padded" : "nts_cigar_rows";
  std::vector<CigTextChain> placed(n_chains);
  auto place = [&](uint64_t c, auto who) -> int { return cig_rows_place(ctx, chains[c], spans[c], a, b, who, placed[c]); };
  if (const int rc = cig_chains_check(ctx, name, CIG_TEXT_MAX_BASES_LOG2, true, chains, n_chains, n_cigar, place)) return rc;
  if (n_cigar == 0) { // (nothing is launched: every row is empty)
    *row_a = nullptr;
    *row_b = nullptr;
    memset(row_first, 0, (n_chains + 1) * 8);
    return NTS_OK;
  }
  // (its own buffers first: while nothing is queued, a request that fails may still return at once)
  NTS_WS(d_placed, CigTextChain*, "cigr_placed", n_chains * sizeof(CigTextChain));
  NTS_WS(d_first, uint64_t*, "cigr_first", (n_chains + 1) * 8);
  std::vector<uint64_t> host_first(n_chains + 1); // (the caller's array is written only when the call succeeds)
  uint32_t worst = SCRIPT_OK;
  CigIndex ix; // columns PA, PB, PC (columns)
  hipError_t e_run;
  auto firsts = [&] { NTS_LAUNCH(k_cig_rows_firsts, IVL_GRID(n_chains + 1), ix.chains, n_chains, n_cigar, ix.column(2), d_first); };
  if (const int rc = cig_index_stage<CigRowsOf<PADDED>>(ctx, "cigar_rows_scan", cigar, n_cigar, chains, n_chains, 0, &worst, ix, e_run, firsts)) return rc;
  if (e_run == hipSuccess) e_run = hipGetLastError();
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(d_placed, placed.data(), n_chains * sizeof(CigTextChain), hipMemcpyHostToDevice, ctx->stream);
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(host_first.data(), d_first, (n_chains + 1) * 8, hipMemcpyDeviceToHost, ctx->stream);
  hipError_t e_sync = hipStreamSynchronize(ctx->stream); // (whatever happened: the caller's arrays were sources of asynchronous copies)
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  if (worst != SCRIPT_OK) return fail(ctx, NTS_EINVAL, std::string(name) + ": the entries of chain " + std::to_string(worst) + " are no CIGAR of its lengths");
  const uint64_t columns = host_first[n_chains];
  if (columns > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, std::string(name) + ": rows of 2^32 columns or more");
  if (columns == 0) { // (checked entries have a column each: kept so that no empty grid is ever launched)
    *row_a = nullptr;
    *row_b = nullptr;
    memset(row_first, 0, (n_chains + 1) * 8);
    return NTS_OK;
  }
  const uint64_t words = (columns + 3) / 4; // (the device buffers are padded to whole words)
  // (the stream is idle: the rows' buffers are fetched before their kernel is queued)
  NTS_WS(d_row_a, uint32_t*, "cigr_row_a", std::max<uint64_t>(words, 1) * 4);
  NTS_WS(d_row_b, uint32_t*, "cigr_row_b", std::max<uint64_t>(words, 1) * 4);
  uint8_t* host_a = (uint8_t*)malloc(std::max<uint64_t>(columns, 1));
  uint8_t* host_b = (uint8_t*)malloc(std::max<uint64_t>(columns, 1));
  if (!host_a || !host_b) {
    free(host_a);
    free(host_b);
    return fail(ctx, NTS_ENOMEM, std::string(name) + ": no host memory for the rows");
  }
  {
    ScopedTimer t(ctx, "cigar_rows_emit", true);
    NTS_LAUNCH(k_cig_rows<PADDED>, IVL_GRID(words), ix.cigar, n_cigar, (const CigTextChain*)d_placed, n_chains, ix.column(0), ix.column(1), ix.column(2),
               (const uint8_t*)a->d_code, a->n + 2 * PAD, (const uint8_t*)b->d_code, b->n + 2 * PAD, d_row_a, d_row_b, words);
  }
  e_run = hipGetLastError();
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(host_a, d_row_a, columns, hipMemcpyDeviceToHost, ctx->stream);
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(host_b, d_row_b, columns, hipMemcpyDeviceToHost, ctx->stream);
  e_sync = hipStreamSynchronize(ctx->stream);
  if (e_run != hipSuccess || e_sync != hipSuccess) {
    free(host_a);
    free(host_b);
  }
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  *row_a = host_a;
  *row_b = host_b;
  memcpy(row_first, host_first.data(), (n_chains + 1) * 8);
  return NTS_OK;
}

// ---- the padded CIGARs of a star alignment: every chain gets the gap columns the other chains' insertions need (nts_cigar_pad) ----
// docs/design/04_30_block_maf_multi.md.  Input: entries and chain records that tile them, and per chain {group, t0}: the chains of one
// GROUP are aligned to one reference record, chain c's A side covering reference bases [t0, t0 + len_a).  SLOT p lies in front of
// reference base p; an I entry that precedes base p sits in slot p; a SITE is a (group, slot) with an I entry, its WIDTH the longest
// such I of the group.  The padded CIGAR of a chain is its entries plus entries of code 6 (P): behind an own I shorter than the width
// the rest of the width, and the whole width at every other site p with t0 <= p < t1 -- in front of the entry that begins at p, or
// splitting the =, X or D run that holds bases p - 1 and p.  No genome is read.
//   1  cig_index_stage with (A bases, B bases, I entries): the third prefix compacts the I entries.  k_cigp_keys: one lane per entry,
//      an I entry stores (group << 32 | slot - R0, len) at its rank; ONE radix sort of the pairs, ONE reduce_by_key with the maximum:
//      the sites, ascending by group and slot, and their widths.  k_cigp_sites: one lane per site (the absolute slot) and one per
//      group and one more (where its sites begin: a lower-bound search) (timer "cigar_pad_sites").
//   2  k_cigp_count: one lane per entry, two lower-bound searches over the site keys give the sites [s_lo, s_hi) of its slots, from
//      which the number of entries it becomes follows without a walk; ONE exclusive scan; k_cig_rows_firsts reads it at every chain's
//      first entry.  k_cigp_emit: ONE LANE PER OUTPUT ENTRY: an upper-bound search over the scan finds its input entry, the same two
//      searches its sites, and its rank r inside the entry says which piece or which P it is -- two site keys or one width are read,
//      whatever the number of sites that cross the run (timer "cigar_pad_emit").
// No atomic, no launch per chain, group or site, no floating point, no host loop over entries or sites (one over chains: the checks).

struct CigPadChain // a chain as the padding kernels read it
{
  uint64_t first; // its first entry
  uint64_t key0;  // group << 32 | t0 - R0 of its group (the extent of a group is below 2^32: host check)
};
static_assert(sizeof(CigPadChain) == 16 && sizeof(nts_cig_pad_at) == 16, "two 8-byte words; the C ABI's layout");

using CigPadTuple = rocprim::tuple<uint64_t, uint64_t, uint64_t>; // A bases, B bases, I entries

struct CigPadOf // element e of the scan's input: what entry e consumes and whether it is an I; nothing behind the last entry
{
  using Tuple = CigPadTuple;
  const uint64_t* cigar;
  uint64_t n_cigar;
  __device__ Tuple operator()(uint64_t e) const
  {
    if (e >= n_cigar) return Tuple(0, 0, 0);
    const uint64_t v = cigar[e];
    const CigBases ab = cig_bases(v);
    return Tuple(rocprim::get<0>(ab), rocprim::get<1>(ab), (v & 15u) == CIG_I ? 1u : 0u);
  }
};

constexpr uint64_t CIGP_MOST = 1ull << 62; // a count of output entries saturates here: no sum of two wraps
struct CigPadSatAdd
{
  __host__ __device__ uint64_t operator()(uint64_t x, uint64_t y) const { return x + y < CIGP_MOST ? x + y : CIGP_MOST; }
};

// the first i < n with key[i] >= k over ascending keys, n where there is none
__device__ __forceinline__ uint64_t cigp_lower(const uint64_t* __restrict__ key, uint64_t n, uint64_t k)
{
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2u;
    if (key[mid] < k) lo = mid + 1u;
    else hi = mid;
  }
  return lo;
}

// the key of the slot in front of entry e: its chain's key0 plus the A bases of the chain in front of e; own: e > the chain's first
__device__ __forceinline__ uint64_t cigp_key_of(const CigPadChain* __restrict__ chains, uint64_t n_chains, const uint64_t* __restrict__ PA, uint64_t e, bool& inner)
{
  const CigPadChain ch = chains[cig_last_at_or_before(n_chains, e, [chains](uint64_t c) { return chains[c].first; })];
  const uint64_t f = ch.first <= e ? ch.first : e;
  inner = e > f;
  return ch.key0 + (PA[e] - PA[f]);
}

// lane e < n_cigar: an I entry stores its (key, length) at its rank among the I entries
__global__ __launch_bounds__(256) void k_cigp_keys(const uint64_t* __restrict__ cigar, uint64_t n_cigar, const CigPadChain* __restrict__ chains,
                                                   uint64_t n_chains, const uint64_t* __restrict__ PA, const uint64_t* __restrict__ PI, uint64_t n_ins,
                                                   uint64_t* __restrict__ key, uint64_t* __restrict__ len)
{
  const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (e >= n_cigar || n_chains == 0) return;
  const uint64_t v = cigar[e];
  if ((v & 15u) != CIG_I) return;
  const uint64_t i = PI[e];
  if (i >= n_ins) return; // (n_ins = PI[n_cigar]: every I entry has a rank below it)
  bool inner;
  key[i] = cigp_key_of(chains, n_chains, PA, e, inner);
  len[i] = v >> 4;
}

// lane i < n_sites: the absolute slot of site i; lane n_sites + g, g <= n_groups: where group g's sites begin
__global__ __launch_bounds__(256) void k_cigp_sites(const uint64_t* __restrict__ site_key, uint64_t n_sites, const uint64_t* __restrict__ r0, uint64_t n_groups,
                                                    uint64_t* __restrict__ site_pos, uint64_t* __restrict__ site_first)
{
  const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (g < n_sites) {
    const uint64_t k = site_key[g], group = k >> 32;
    site_pos[g] = (group < n_groups ? r0[group] : 0) + (k & 0xFFFFFFFFull);
  } else if (g - n_sites <= n_groups) {
    site_first[g - n_sites] = cigp_lower(site_key, n_sites, (g - n_sites) << 32);
  }
}

struct CigPadPlan // what entry e becomes: its sites [s_lo, s_hi) and whether the first of them lies in front of its first base
{
  uint64_t v, key0, s_lo, s_hi;
  uint32_t has0;
  __device__ __forceinline__ uint64_t count(const uint64_t* __restrict__ site_w) const
  {
    if ((v & 15u) == CIG_I) return 1u + (s_lo < s_hi && site_w[s_lo] > (v >> 4) ? 1u : 0u); // the I, and the rest of the width
    return 2u * (s_hi - s_lo) - has0 + 1u; // a P per site, a piece in front of every inner site and one behind the last
  }
};

__device__ __forceinline__ CigPadPlan cigp_plan(const uint64_t* __restrict__ cigar, const CigPadChain* __restrict__ chains, uint64_t n_chains,
                                                const uint64_t* __restrict__ PA, const uint64_t* __restrict__ site_key, uint64_t n_sites, uint64_t e)
{
  CigPadPlan p;
  p.v = cigar[e];
  bool inner;
  p.key0 = cigp_key_of(chains, n_chains, PA, e, inner);
  if ((p.v & 15u) == CIG_I) { // its own site (k_cigp_keys stored this key: it is there)
    p.s_lo = cigp_lower(site_key, n_sites, p.key0);
    p.s_hi = p.s_lo + (p.s_lo < n_sites && site_key[p.s_lo] == p.key0 ? 1u : 0u);
    p.has0 = 0;
  } else { // =, X, D: len A bases; the slot in front of it is the I's in front of it where the chain has one there
    const bool own = inner && (cigar[e - 1u] & 15u) == CIG_I;
    p.s_lo = cigp_lower(site_key, n_sites, p.key0 + (own ? 1u : 0u));
    p.s_hi = cigp_lower(site_key, n_sites, p.key0 + (p.v >> 4));
    if (p.s_hi < p.s_lo) p.s_hi = p.s_lo; // (ascending keys: never)
    p.has0 = !own && p.s_lo < p.s_hi && site_key[p.s_lo] == p.key0 ? 1u : 0u;
  }
  return p;
}

// lane e <= n_cigar: the number of entries that entry e becomes, 0 behind the last
__global__ __launch_bounds__(256) void k_cigp_count(const uint64_t* __restrict__ cigar, uint64_t n_cigar, const CigPadChain* __restrict__ chains,
                                                    uint64_t n_chains, const uint64_t* __restrict__ PA, const uint64_t* __restrict__ site_key,
                                                    const uint64_t* __restrict__ site_w, uint64_t n_sites, uint64_t* __restrict__ count)
{
  const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (e > n_cigar) return;
  count[e] = e < n_cigar && n_chains ? cigp_plan(cigar, chains, n_chains, PA, site_key, n_sites, e).count(site_w) : 0;
}

// lane o < n_out: output entry o
__global__ __launch_bounds__(256) void k_cigp_emit(const uint64_t* __restrict__ cigar, uint64_t n_cigar, const CigPadChain* __restrict__ chains,
                                                   uint64_t n_chains, const uint64_t* __restrict__ PA, const uint64_t* __restrict__ PO,
                                                   const uint64_t* __restrict__ site_key, const uint64_t* __restrict__ site_w, uint64_t n_sites,
                                                   uint64_t* __restrict__ out, uint64_t n_out)
{
  const uint64_t o = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (o >= n_out || n_cigar == 0 || n_chains == 0) return;
  const uint64_t e = cig_last_at_or_before(n_cigar, o, [PO](uint64_t i) { return PO[i]; }); // (PO[0] = 0 <= o; every entry becomes at least one)
  const CigPadPlan p = cigp_plan(cigar, chains, n_chains, PA, site_key, n_sites, e);
  const uint64_t r = o - PO[e], code = p.v & 15u, len = p.v >> 4;
  uint64_t say = 0; // (an entry of length 0: no reader takes it; only where the scan and the plan disagree, which they do not)
  if (r >= p.count(site_w)) {
  } else if (code == CIG_I) {
    say = r == 0 ? p.v : (site_w[p.s_lo] - len) << 4 | CIG_P;
  } else if (p.has0 && r == 0) {
    say = site_w[p.s_lo] << 4 | CIG_P;
  } else {
    const uint64_t k = r - p.has0, q = k >> 1, base = p.s_lo + p.has0, inside = p.s_hi - base; // piece q or the P behind it; base: the first inner site
    if (k & 1u) {
      say = site_w[base + q] << 4 | CIG_P; // (k = 2 q + 1 <= 2 inside: q < inside)
    } else {
      const uint64_t from = q == 0 ? p.key0 : site_key[base + q - 1u], to = q >= inside ? p.key0 + len : site_key[base + q];
      say = (to - from) << 4 | code;
    }
  }
  out[o] = say;
}

int cigar_pad_run(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains, const nts_cig_pad_at* at,
                  uint64_t n_groups, uint64_t** padded, uint64_t* pad_first, uint64_t* site_first, uint64_t** site_pos, uint64_t** site_w)
{
  std::vector<CigPadChain> placed;
  std::vector<uint64_t> r0;
  try {
    placed.resize(n_chains);
    r0.assign(std::max<uint64_t>(n_groups, 1), 0);
  } catch (const std::bad_alloc&) {
    return fail(ctx, NTS_ENOMEM, "nts_cigar_pad: no host memory for the chains and groups");
  }
  uint64_t lo = 0, hi = 0; // the extent of the group of the chain in front
  auto place = [&](uint64_t c, auto who) -> int {
    const nts_cig_chain& ch = chains[c];
    const nts_cig_pad_at& a = at[c];
    if (a.group >= n_groups) return fail(ctx, NTS_EINVAL, who() + " names a group outside n_groups");
    if (c && a.group < at[c - 1].group) return fail(ctx, NTS_EINVAL, who() + ": the groups are not nondecreasing");
    if (ch.n_cig) {
      const uint64_t head = cigar[ch.first] & 15u, tail = cigar[ch.first + ch.n_cig - 1u] & 15u;
      if ((head != CIG_EQ && head != CIG_X) || (tail != CIG_EQ && tail != CIG_X))
        return fail(ctx, NTS_EINVAL, who() + ": its first or last entry is not = or X (pad the core of a chain)");
    }
    if (a.t0 > ~0ull - ch.len_a) return fail(ctx, NTS_ERANGE, who() + ": t0 + len_a wraps");
    const bool opens = c == 0 || a.group != at[c - 1].group;
    lo = opens ? a.t0 : std::min(lo, a.t0);
    hi = opens ? a.t0 + ch.len_a : std::max(hi, a.t0 + ch.len_a);
    if (hi - lo > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, who() + ": the reference extent of its group is 2^32 or more");
    r0[a.group] = lo;
    placed[c] = { ch.first, a.t0 }; // (the key once every chain of the group is seen: below)
    return NTS_OK;
  };
  if (const int rc = cig_chains_check(ctx, "nts_cigar_pad", CIG_TEXT_MAX_BASES_LOG2, true, chains, n_chains, n_cigar, place)) return rc;
  for (uint64_t c = 0; c < n_chains; ++c) placed[c].key0 = ((uint64_t)at[c].group << 32) + (placed[c].key0 - r0[at[c].group]);
  auto nothing = [&] {
    *padded = nullptr;
    *site_pos = nullptr;
    *site_w = nullptr;
    memset(pad_first, 0, (n_chains + 1) * 8);
    memset(site_first, 0, (n_groups + 1) * 8);
    return NTS_OK;
  };
  if (n_cigar == 0) return nothing(); // (nothing is launched)
  // (its own buffers first: while nothing is queued, a request that fails may still return at once)
  NTS_WS(d_placed, CigPadChain*, "cigp_placed", n_chains * sizeof(CigPadChain));
  NTS_WS(d_r0, uint64_t*, "cigp_r0", std::max<uint64_t>(n_groups, 1) * 8);
  NTS_WS(d_count, uint64_t*, "cigp_count", (n_cigar + 1) * 8);
  NTS_WS(d_po, uint64_t*, "cigp_po", (n_cigar + 1) * 8);
  NTS_WS(d_pad_first, uint64_t*, "cigp_pad_first", (n_chains + 1) * 8);
  NTS_WS(d_site_first, uint64_t*, "cigp_site_first", (n_groups + 1) * 8);
  NTS_WS(d_num, uint64_t*, "cigp_num", 8);
  uint32_t worst = SCRIPT_OK;
  uint64_t n_ins = 0, n_sites = 0;
  CigIndex ix; // columns PA, PB, PI (I entries)
  hipError_t e_run;
  if (const int rc = cig_index_stage<CigPadOf>(ctx, "cigar_pad_sites", cigar, n_cigar, chains, n_chains, 0, &worst, ix, e_run, [] {})) return rc;
  if (e_run == hipSuccess) e_run = hipGetLastError();
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(d_placed, placed.data(), n_chains * sizeof(CigPadChain), hipMemcpyHostToDevice, ctx->stream);
  if (e_run == hipSuccess && n_groups) e_run = hipMemcpyAsync(d_r0, r0.data(), n_groups * 8, hipMemcpyHostToDevice, ctx->stream);
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(&n_ins, ix.column(2) + n_cigar, 8, hipMemcpyDeviceToHost, ctx->stream);
  hipError_t e_sync = hipStreamSynchronize(ctx->stream); // (whatever happened: the caller's arrays were sources of asynchronous copies)
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  if (worst != SCRIPT_OK) {
    if (worst < n_chains) // (the error path alone looks at the entries of that one chain)
      for (uint64_t e = chains[worst].first; e < chains[worst].first + chains[worst].n_cig; ++e)
        if ((cigar[e] & 15u) == CIG_P)
          return fail(ctx, NTS_EINVAL, "nts_cigar_pad: chain " + std::to_string(worst) + " holds an entry of code 6: it is padded already");
    return fail(ctx, NTS_EINVAL, "nts_cigar_pad: the entries of chain " + std::to_string(worst) + " are no CIGAR of its lengths");
  }
  if (n_ins > n_cigar) return fail(ctx, NTS_EHIP, "nts_cigar_pad: the scan counted more I entries than there are entries");
  // (the stream is idle: the buffers sized by the I entries are fetched before their kernels are queued)
  const uint64_t cap = std::max<uint64_t>(n_ins, 1);
  NTS_WS(d_key, uint64_t*, "cigp_key", cap * 8);
  NTS_WS(d_len, uint64_t*, "cigp_len", cap * 8);
  NTS_WS(d_key2, uint64_t*, "cigp_key2", cap * 8);
  NTS_WS(d_len2, uint64_t*, "cigp_len2", cap * 8);
  NTS_WS(d_site_key, uint64_t*, "cigp_site_key", cap * 8);
  NTS_WS(d_site_w, uint64_t*, "cigp_site_w", cap * 8);
  NTS_WS(d_site_pos, uint64_t*, "cigp_site_pos", cap * 8);
  size_t tmp_sort = 0, tmp_red = 0, tmp_scan = 0;
  if (n_ins) {
    e_run = rocprim::radix_sort_pairs(nullptr, tmp_sort, d_key, d_key2, d_len, d_len2, n_ins, 0, 64, ctx->stream);
    if (e_run == hipSuccess)
      e_run = rocprim::reduce_by_key(nullptr, tmp_red, d_key2, d_len2, n_ins, d_site_key, d_site_w, d_num, rocprim::maximum<uint64_t>(),
                                     rocprim::equal_to<uint64_t>(), ctx->stream);
  }
  if (e_run == hipSuccess) e_run = rocprim::exclusive_scan(nullptr, tmp_scan, d_count, d_po, (uint64_t)0, n_cigar + 1, CigPadSatAdd(), ctx->stream);
  HIP_TRY(ctx, e_run);
  NTS_WS(d_tmp, void*, "ivs_tmp", std::max<size_t>(std::max(tmp_sort, std::max(tmp_red, tmp_scan)), 16)); // (ix.tmp is dead from here)
  if (n_ins) {
    {
      ScopedTimer t(ctx, "cigar_pad_sites", true);
      NTS_LAUNCH(k_cigp_keys, IVL_GRID(n_cigar), ix.cigar, n_cigar, (const CigPadChain*)d_placed, n_chains, ix.column(0), ix.column(2), n_ins, d_key, d_len);
      e_run = rocprim::radix_sort_pairs(d_tmp, tmp_sort, d_key, d_key2, d_len, d_len2, n_ins, 0, 64, ctx->stream);
      if (e_run == hipSuccess)
        e_run = rocprim::reduce_by_key(d_tmp, tmp_red, d_key2, d_len2, n_ins, d_site_key, d_site_w, d_num, rocprim::maximum<uint64_t>(),
                                       rocprim::equal_to<uint64_t>(), ctx->stream);
    }
    if (e_run == hipSuccess) e_run = hipGetLastError();
    if (e_run == hipSuccess) e_run = hipMemcpyAsync(&n_sites, d_num, 8, hipMemcpyDeviceToHost, ctx->stream);
    e_sync = hipStreamSynchronize(ctx->stream);
    HIP_TRY(ctx, e_run);
    HIP_TRY(ctx, e_sync);
    if (n_sites == 0 || n_sites > n_ins) return fail(ctx, NTS_EHIP, "nts_cigar_pad: the reduction left an impossible number of sites");
  }
  std::vector<uint64_t> host_pad_first(n_chains + 1), host_site_first(n_groups + 1); // (the caller's arrays are written only when the call succeeds)
  {
    ScopedTimer t(ctx, "cigar_pad_sites", true);
    NTS_LAUNCH(k_cigp_sites, IVL_GRID(n_sites + n_groups + 1), (const uint64_t*)d_site_key, n_sites, (const uint64_t*)d_r0, n_groups, d_site_pos, d_site_first);
  }
  {
    ScopedTimer t(ctx, "cigar_pad_emit", true);
    NTS_LAUNCH(k_cigp_count, IVL_GRID(n_cigar + 1), ix.cigar, n_cigar, (const CigPadChain*)d_placed, n_chains, ix.column(0), (const uint64_t*)d_site_key,
               (const uint64_t*)d_site_w, n_sites, d_count);
    e_run = rocprim::exclusive_scan(d_tmp, tmp_scan, d_count, d_po, (uint64_t)0, n_cigar + 1, CigPadSatAdd(), ctx->stream);
    if (e_run == hipSuccess) NTS_LAUNCH(k_cig_rows_firsts, IVL_GRID(n_chains + 1), ix.chains, n_chains, n_cigar, (const uint64_t*)d_po, d_pad_first);
  }
  if (e_run == hipSuccess) e_run = hipGetLastError();
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(host_pad_first.data(), d_pad_first, (n_chains + 1) * 8, hipMemcpyDeviceToHost, ctx->stream);
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(host_site_first.data(), d_site_first, (n_groups + 1) * 8, hipMemcpyDeviceToHost, ctx->stream);
  e_sync = hipStreamSynchronize(ctx->stream);
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  const uint64_t n_out = host_pad_first[n_chains];
  if (n_out > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, "nts_cigar_pad: 2^32 output entries or more");
  if (n_out < n_cigar || host_site_first[n_groups] != n_sites) return fail(ctx, NTS_EHIP, "nts_cigar_pad: the scan left impossible totals");
  // (the stream is idle: the output's buffer is fetched before its kernel is queued)
  NTS_WS(d_out, uint64_t*, "cigp_out", n_out * 8);
  uint64_t* host_out = (uint64_t*)malloc(n_out * 8);
  uint64_t* host_pos = n_sites ? (uint64_t*)malloc(n_sites * 8) : nullptr;
  uint64_t* host_w = n_sites ? (uint64_t*)malloc(n_sites * 8) : nullptr;
  auto drop = [&] {
    free(host_out);
    free(host_pos);
    free(host_w);
  };
  if (!host_out || (n_sites && (!host_pos || !host_w))) {
    drop();
    return fail(ctx, NTS_ENOMEM, "nts_cigar_pad: no host memory for the padded entries");
  }
  {
    ScopedTimer t(ctx, "cigar_pad_emit", true);
    NTS_LAUNCH(k_cigp_emit, IVL_GRID(n_out), ix.cigar, n_cigar, (const CigPadChain*)d_placed, n_chains, ix.column(0), (const uint64_t*)d_po,
               (const uint64_t*)d_site_key, (const uint64_t*)d_site_w, n_sites, d_out, n_out);
  }
  e_run = hipGetLastError();
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(host_out, d_out, n_out * 8, hipMemcpyDeviceToHost, ctx->stream);
  if (e_run == hipSuccess && n_sites) e_run = hipMemcpyAsync(host_pos, d_site_pos, n_sites * 8, hipMemcpyDeviceToHost, ctx->stream);
  if (e_run == hipSuccess && n_sites) e_run = hipMemcpyAsync(host_w, d_site_w, n_sites * 8, hipMemcpyDeviceToHost, ctx->stream);
  e_sync = hipStreamSynchronize(ctx->stream);
  if (e_run != hipSuccess || e_sync != hipSuccess) drop();
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  *padded = host_out;
  *site_pos = host_pos;
  *site_w = host_w;
  memcpy(pad_first, host_pad_first.data(), (n_chains + 1) * 8);
  memcpy(site_first, host_site_first.data(), (n_groups + 1) * 8);
  return NTS_OK;
}

// ---- per-base depth and identity over a star alignment: the segments of constant (aligned, match, gap) (nts_cigar_depth) ----
// docs/design/04_31_block_conservation.md.  Input as nts_cigar_pad's -- entries, chain records that tile them, {group, t0} per chain --
// but the chains need not be cores, the entries need not be maximal runs, and chains of one group may overlap freely.  For a group g
// and a reference base p: aligned = the chains of g that cover p, match = those in which p lies in an = entry, gap = those in which
// it lies in a D entry.  A SEGMENT is a maximal run of reference bases of one group with aligned > 0 and one triple.  No genome is read.
//   1  cig_index_stage with (A bases, B bases, consuming entries): the third prefix PC ranks the =, X and D entries.  k_cigd_events:
//      one lane per entry and one per chain.  A consuming entry stores ONE event at its rank: key group << 32 | the base it begins at
//      - R0, value the state it enters minus the state of the consuming entry in front of it in its chain (nothing in front: the state
//      alone, which opens the chain); chain c stores one closing event at slot n_consuming + c: key t1, value minus the state of its
//      last consuming entry (0 where it has none).  A state is three counts in one 64-bit word, 21 bits each, added modulo 2^64: exact
//      where every true count is below 2^21, and a group holds fewer than 2^20 chains.  ONE radix sort of the pairs, ONE reduce_by_key
//      with the sum: the distinct boundaries, ascending by group and base, and their net deltas (timer "cigar_depth_events").
//   2  ONE inclusive scan of the deltas over ALL boundaries (every group closes to zero): the state of the stretch behind each.
//      k_cigd_heads: one lane per boundary; its stretch is LIVE when the next boundary is of its group and aligned > 0, and a HEAD
//      when the stretch in front is not live or has another triple.  ONE exclusive scan of the heads.  k_cigd_firsts: one lane per
//      group and one more, a lower-bound search over the boundary keys.  k_cigd_emit: one lane per boundary; a head writes start,
//      group and triple at its rank, the last live stretch of a run writes end (timer "cigar_depth_emit").
// No atomic, no launch per chain, group or segment, no floating point, no host loop over entries, events or segments (one over
// chains: the checks and R0).

static_assert(sizeof(nts_cig_depth_seg) == 32, "the C ABI's layout");

constexpr uint32_t CIGD_FIELD = 21;                         // bits per count
constexpr uint64_t CIGD_MASK = (1ull << CIGD_FIELD) - 1u;
constexpr uint64_t CIGD_MOST_CHAINS = 1ull << 20;           // a group of that many chains is refused: a count might leave its field
constexpr uint64_t CIGD_ALIGNED = 1ull, CIGD_MATCH = 1ull << CIGD_FIELD, CIGD_GAP = 1ull << (2 * CIGD_FIELD);
constexpr uint64_t CIGD_BAD = 1ull << 63, CIGD_RANK = (1ull << 40) - 1u; // a head count: its rank below 2^40, and whether a group did not close

__host__ __device__ inline bool cigd_consumes(uint64_t v)
{
  const uint64_t code = v & 15u;
  return code == CIG_EQ || code == CIG_X || code == CIG_D;
}

// what a chain adds to the counts of the reference bases of a consuming entry
__device__ __forceinline__ uint64_t cigd_state(uint64_t v)
{
  const uint64_t code = v & 15u;
  return CIGD_ALIGNED + (code == CIG_EQ ? CIGD_MATCH : 0u) + (code == CIG_D ? CIGD_GAP : 0u);
}

using CigDepthTuple = rocprim::tuple<uint64_t, uint64_t, uint64_t>; // A bases, B bases, consuming entries

struct CigDepthOf // element e of the scan's input: what entry e consumes and whether it consumes reference bases; nothing behind the last entry
{
  using Tuple = CigDepthTuple;
  const uint64_t* cigar;
  uint64_t n_cigar;
  __device__ Tuple operator()(uint64_t e) const
  {
    if (e >= n_cigar) return Tuple(0, 0, 0);
    const uint64_t v = cigar[e];
    const CigBases ab = cig_bases(v);
    return Tuple(rocprim::get<0>(ab), rocprim::get<1>(ab), cigd_consumes(v) ? 1u : 0u);
  }
};

struct CigDepthHeadAdd // ranks add (below 2^40: there are fewer than 2^34 boundaries), the flag of a group that did not close is kept
{
  __host__ __device__ uint64_t operator()(uint64_t x, uint64_t y) const { return (((x & CIGD_RANK) + (y & CIGD_RANK)) & CIGD_RANK) | ((x | y) & CIGD_BAD); }
};

// the consuming entry of rank r among entries [lo, hi) with PC[lo] <= r < PC[hi]: the last e with PC[e] <= r
__device__ __forceinline__ uint64_t cigd_entry_of_rank(const uint64_t* __restrict__ PC, uint64_t lo, uint64_t hi, uint64_t r)
{
  while (hi - lo > 1u) {
    const uint64_t mid = lo + (hi - lo) / 2u;
    if (PC[mid] <= r) lo = mid;
    else hi = mid;
  }
  return lo;
}

// lane e < n_cigar: a consuming entry stores its event at its rank; lane n_cigar + c: chain c's closing event at slot n_cons + c
__global__ __launch_bounds__(256) void k_cigd_events(const uint64_t* __restrict__ cigar, uint64_t n_cigar, const CigPadChain* __restrict__ placed,
                                                     const nts_cig_chain* __restrict__ chains, uint64_t n_chains, const uint64_t* __restrict__ PA,
                                                     const uint64_t* __restrict__ PC, uint64_t n_cons, uint64_t* __restrict__ key,
                                                     uint64_t* __restrict__ val)
{
  const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (g >= n_cigar + n_chains || n_chains == 0) return;
  if (g < n_cigar) {
    const uint64_t v = cigar[g];
    if (!cigd_consumes(v)) return;
    const uint64_t i = PC[g];
    if (i >= n_cons) return; // (n_cons = PC[n_cigar]: every consuming entry has a rank below it)
    const CigPadChain ch = placed[cig_last_at_or_before(n_chains, g, [placed](uint64_t c) { return placed[c].first; })];
    const uint64_t f = ch.first <= g ? ch.first : g;
    uint64_t before = 0; // the state of the consuming entry in front of it in its chain
    if (i > PC[f]) {
      const uint64_t p = cigd_consumes(cigar[g - 1u]) ? g - 1u : cigd_entry_of_rank(PC, f, g, i - 1u); // (i > PC[f]: g > f)
      before = cigd_state(cigar[p]);
    }
    key[i] = ch.key0 + (PA[g] - PA[f]);
    val[i] = cigd_state(v) - before;
  } else {
    const uint64_t c = g - n_cigar;
    const nts_cig_chain ch = chains[c];
    uint64_t k = placed[c].key0, last = 0;
    if (!cig_chain_beyond(ch, n_cigar)) {
      const uint64_t end = ch.first + ch.n_cig;
      k += PA[end] - PA[ch.first];
      if (PC[end] > PC[ch.first]) last = cigd_state(cigar[cigd_entry_of_rank(PC, ch.first, end, PC[end] - 1u)]);
    }
    key[n_cons + c] = k; // (n_cons + n_chains words)
    val[n_cons + c] = 0u - last;
  }
}

// whether the stretch behind boundary i is live: the next boundary is of its group and some chain covers it
__device__ __forceinline__ bool cigd_live(const uint64_t* __restrict__ bkey, const uint64_t* __restrict__ state, uint64_t n_b, uint64_t i)
{
  return i + 1u < n_b && (bkey[i + 1u] >> 32) == (bkey[i] >> 32) && (state[i] & CIGD_MASK) != 0;
}

// whether the live stretch behind boundary i opens a segment: the stretch in front is not live (or of another group: then it is not) or has another triple
__device__ __forceinline__ bool cigd_head(const uint64_t* __restrict__ bkey, const uint64_t* __restrict__ state, uint64_t n_b, uint64_t i)
{
  return !(i > 0 && cigd_live(bkey, state, n_b, i - 1u) && state[i - 1u] == state[i]);
}

// lane i < n_b: 1 for a head, and the flag of a group that ends with a state other than zero; lane n_b: 0
__global__ __launch_bounds__(256) void k_cigd_heads(const uint64_t* __restrict__ bkey, const uint64_t* __restrict__ state, uint64_t n_b,
                                                    uint64_t* __restrict__ head)
{
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i > n_b) return;
  uint64_t say = 0;
  if (i < n_b) {
    if (cigd_live(bkey, state, n_b, i) && cigd_head(bkey, state, n_b, i)) say = 1u;
    if ((i + 1u == n_b || (bkey[i + 1u] >> 32) != (bkey[i] >> 32)) && state[i] != 0) say |= CIGD_BAD;
  }
  head[i] = say; // (n_b + 1 words)
}

// lane g <= n_groups: where group g's segments begin; lane n_groups + 1: whether some group did not close
__global__ __launch_bounds__(256) void k_cigd_firsts(const uint64_t* __restrict__ bkey, uint64_t n_b, const uint64_t* __restrict__ rank, uint64_t n_groups,
                                                     uint64_t* __restrict__ seg_first)
{
  const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (g <= n_groups) seg_first[g] = rank[cigp_lower(bkey, n_b, g << 32)] & CIGD_RANK; // (cigp_lower <= n_b; rank: n_b + 1 words)
  else if (g == n_groups + 1u) seg_first[g] = rank[n_b] >> 63;                     // (n_groups + 2 words)
}

// lane i < n_b: a head writes its segment's start, group and triple; the last live stretch of a run writes its end
__global__ __launch_bounds__(256) void k_cigd_emit(const uint64_t* __restrict__ bkey, const uint64_t* __restrict__ state, uint64_t n_b,
                                                   const uint64_t* __restrict__ rank, const uint64_t* __restrict__ r0, uint64_t n_groups,
                                                   nts_cig_depth_seg* __restrict__ segs, uint64_t n_segs)
{
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n_b || !cigd_live(bkey, state, n_b, i)) return;
  const uint64_t k = bkey[i], group = k >> 32, s = state[i];
  const uint64_t base = group < n_groups ? r0[group] : 0;
  const uint64_t r = (rank[i + 1u] & CIGD_RANK) - 1u; // the heads up to and with this stretch, less one: the head of its run (0 - 1: beyond n_segs)
  if (r >= n_segs) return;
  if (cigd_head(bkey, state, n_b, i)) {
    segs[r].start = base + (k & 0xFFFFFFFFull);
    segs[r].group = (uint32_t)group;
    segs[r].aligned = (uint32_t)(s & CIGD_MASK);
    segs[r].match = (uint32_t)(s >> CIGD_FIELD & CIGD_MASK);
    segs[r].gap = (uint32_t)(s >> (2 * CIGD_FIELD) & CIGD_MASK);
  }
  if (!(cigd_live(bkey, state, n_b, i + 1u) && state[i + 1u] == s)) segs[r].end = base + (bkey[i + 1u] & 0xFFFFFFFFull); // (live: i + 1 < n_b)
}

int cigar_depth_run(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains, const nts_cig_pad_at* at,
                    uint64_t n_groups, nts_cig_depth_seg** segs, uint64_t* seg_first)
{
  std::vector<CigPadChain> placed;
  std::vector<uint64_t> r0;
  try {
    placed.resize(n_chains);
    r0.assign(std::max<uint64_t>(n_groups, 1), 0);
  } catch (const std::bad_alloc&) {
    return fail(ctx, NTS_ENOMEM, "nts_cigar_depth: no host memory for the chains and groups");
  }
  uint64_t lo = 0, hi = 0, members = 0; // the extent and the chains of the group of the chain in front
  auto place = [&](uint64_t c, auto who) -> int {
    const nts_cig_chain& ch = chains[c];
    const nts_cig_pad_at& a = at[c];
    if (a.group >= n_groups) return fail(ctx, NTS_EINVAL, who() + " names a group outside n_groups");
    if (c && a.group < at[c - 1].group) return fail(ctx, NTS_EINVAL, who() + ": the groups are not nondecreasing");
    if (a.t0 > ~0ull - ch.len_a) return fail(ctx, NTS_ERANGE, who() + ": t0 + len_a wraps");
    const bool opens = c == 0 || a.group != at[c - 1].group;
    lo = opens ? a.t0 : std::min(lo, a.t0);
    hi = opens ? a.t0 + ch.len_a : std::max(hi, a.t0 + ch.len_a);
    members = opens ? 1 : members + 1;
    if (hi - lo > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, who() + ": the reference extent of its group is 2^32 or more");
    if (members >= CIGD_MOST_CHAINS) return fail(ctx, NTS_ERANGE, who() + ": its group has 2^20 chains or more");
    r0[a.group] = lo;
    placed[c] = { ch.first, a.t0 }; // (the key once every chain of the group is seen: below)
    return NTS_OK;
  };
  if (const int rc = cig_chains_check(ctx, "nts_cigar_depth", CIG_TEXT_MAX_BASES_LOG2, true, chains, n_chains, n_cigar, place)) return rc;
  for (uint64_t c = 0; c < n_chains; ++c) placed[c].key0 = ((uint64_t)at[c].group << 32) + (placed[c].key0 - r0[at[c].group]);
  if (n_cigar == 0) { // (nothing is launched)
    *segs = nullptr;
    memset(seg_first, 0, (n_groups + 1) * 8);
    return NTS_OK;
  }
  // (its own buffers first: while nothing is queued, a request that fails may still return at once)
  NTS_WS(d_placed, CigPadChain*, "cigd_placed", n_chains * sizeof(CigPadChain));
  NTS_WS(d_r0, uint64_t*, "cigd_r0", std::max<uint64_t>(n_groups, 1) * 8);
  NTS_WS(d_seg_first, uint64_t*, "cigd_seg_first", (n_groups + 2) * 8);
  NTS_WS(d_num, uint64_t*, "cigd_num", 8);
  uint32_t worst = SCRIPT_OK;
  uint64_t n_cons = 0, n_b = 0;
  CigIndex ix; // columns PA, PB, PC (consuming entries)
  hipError_t e_run;
  if (const int rc = cig_index_stage<CigDepthOf>(ctx, "cigar_depth_events", cigar, n_cigar, chains, n_chains, 0, &worst, ix, e_run, [] {})) return rc;
  if (e_run == hipSuccess) e_run = hipGetLastError();
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(d_placed, placed.data(), n_chains * sizeof(CigPadChain), hipMemcpyHostToDevice, ctx->stream);
  if (e_run == hipSuccess && n_groups) e_run = hipMemcpyAsync(d_r0, r0.data(), n_groups * 8, hipMemcpyHostToDevice, ctx->stream);
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(&n_cons, ix.column(2) + n_cigar, 8, hipMemcpyDeviceToHost, ctx->stream);
  hipError_t e_sync = hipStreamSynchronize(ctx->stream); // (whatever happened: the caller's arrays were sources of asynchronous copies)
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  if (worst != SCRIPT_OK) {
    if (worst < n_chains) // (the error path alone looks at the entries of that one chain)
      for (uint64_t e = chains[worst].first; e < chains[worst].first + chains[worst].n_cig; ++e)
        if ((cigar[e] & 15u) == CIG_P) return fail(ctx, NTS_EINVAL, "nts_cigar_depth: chain " + std::to_string(worst) + " holds an entry of code 6");
    return fail(ctx, NTS_EINVAL, "nts_cigar_depth: the entries of chain " + std::to_string(worst) + " are no CIGAR of its lengths");
  }
  if (n_cons > n_cigar) return fail(ctx, NTS_EHIP, "nts_cigar_depth: the scan counted more consuming entries than there are entries");
  // (the stream is idle: the buffers sized by the events are fetched before their kernels are queued)
  const uint64_t n_ev = n_cons + n_chains; // (>= 1: entries have a chain)
  NTS_WS(d_key, uint64_t*, "cigd_key", n_ev * 8);
  NTS_WS(d_val, uint64_t*, "cigd_val", n_ev * 8);
  NTS_WS(d_key2, uint64_t*, "cigd_key2", n_ev * 8);
  NTS_WS(d_val2, uint64_t*, "cigd_val2", n_ev * 8);
  NTS_WS(d_bkey, uint64_t*, "cigd_bkey", n_ev * 8);
  NTS_WS(d_delta, uint64_t*, "cigd_delta", n_ev * 8);
  NTS_WS(d_state, uint64_t*, "cigd_state", n_ev * 8);
  NTS_WS(d_head, uint64_t*, "cigd_head", (n_ev + 1) * 8);
  NTS_WS(d_rank, uint64_t*, "cigd_rank", (n_ev + 1) * 8);
  size_t tmp_sort = 0, tmp_red = 0, tmp_scan = 0, tmp_ranks = 0;
  e_run = rocprim::radix_sort_pairs(nullptr, tmp_sort, d_key, d_key2, d_val, d_val2, n_ev, 0, 64, ctx->stream);
  if (e_run == hipSuccess)
    e_run = rocprim::reduce_by_key(nullptr, tmp_red, d_key2, d_val2, n_ev, d_bkey, d_delta, d_num, rocprim::plus<uint64_t>(), rocprim::equal_to<uint64_t>(),
                                   ctx->stream);
  if (e_run == hipSuccess) e_run = rocprim::inclusive_scan(nullptr, tmp_scan, d_delta, d_state, n_ev, rocprim::plus<uint64_t>(), ctx->stream);
  if (e_run == hipSuccess) e_run = rocprim::exclusive_scan(nullptr, tmp_ranks, d_head, d_rank, (uint64_t)0, n_ev + 1, CigDepthHeadAdd(), ctx->stream);
  HIP_TRY(ctx, e_run);
  NTS_WS(d_tmp, void*, "ivs_tmp", std::max<size_t>(std::max(std::max(tmp_sort, tmp_red), std::max(tmp_scan, tmp_ranks)), 16)); // (ix.tmp is dead from here)
  {
    ScopedTimer t(ctx, "cigar_depth_events", true);
    NTS_LAUNCH(k_cigd_events, IVL_GRID(n_cigar + n_chains), ix.cigar, n_cigar, (const CigPadChain*)d_placed, ix.chains, n_chains, ix.column(0), ix.column(2),
               n_cons, d_key, d_val);
    e_run = rocprim::radix_sort_pairs(d_tmp, tmp_sort, d_key, d_key2, d_val, d_val2, n_ev, 0, 64, ctx->stream);
    if (e_run == hipSuccess)
      e_run = rocprim::reduce_by_key(d_tmp, tmp_red, d_key2, d_val2, n_ev, d_bkey, d_delta, d_num, rocprim::plus<uint64_t>(), rocprim::equal_to<uint64_t>(),
                                     ctx->stream);
  }
  if (e_run == hipSuccess) e_run = hipGetLastError();
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(&n_b, d_num, 8, hipMemcpyDeviceToHost, ctx->stream);
  e_sync = hipStreamSynchronize(ctx->stream);
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  if (n_b == 0 || n_b > n_ev) return fail(ctx, NTS_EHIP, "nts_cigar_depth: the reduction left an impossible number of boundaries");
  std::vector<uint64_t> host_seg_first(n_groups + 2); // (the caller's array is written only when the call succeeds)
  {
    ScopedTimer t(ctx, "cigar_depth_emit", true);
    e_run = rocprim::inclusive_scan(d_tmp, tmp_scan, d_delta, d_state, n_b, rocprim::plus<uint64_t>(), ctx->stream);
    if (e_run == hipSuccess) {
      NTS_LAUNCH(k_cigd_heads, IVL_GRID(n_b + 1), (const uint64_t*)d_bkey, (const uint64_t*)d_state, n_b, d_head);
      e_run = rocprim::exclusive_scan(d_tmp, tmp_ranks, d_head, d_rank, (uint64_t)0, n_b + 1, CigDepthHeadAdd(), ctx->stream);
    }
    if (e_run == hipSuccess)
      NTS_LAUNCH(k_cigd_firsts, IVL_GRID(n_groups + 2), (const uint64_t*)d_bkey, n_b, (const uint64_t*)d_rank, n_groups, d_seg_first);
  }
  if (e_run == hipSuccess) e_run = hipGetLastError();
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(host_seg_first.data(), d_seg_first, (n_groups + 2) * 8, hipMemcpyDeviceToHost, ctx->stream);
  e_sync = hipStreamSynchronize(ctx->stream);
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  const uint64_t n_segs = host_seg_first[n_groups];
  if (host_seg_first[n_groups + 1]) return fail(ctx, NTS_EHIP, "nts_cigar_depth: a group does not close to zero");
  if (n_segs > n_b) return fail(ctx, NTS_EHIP, "nts_cigar_depth: the scan left an impossible number of segments");
  nts_cig_depth_seg* host_segs = nullptr;
  if (n_segs) {
    // (the stream is idle: the output's buffer is fetched before its kernel is queued)
    NTS_WS(d_segs, nts_cig_depth_seg*, "cigd_segs", n_segs * sizeof(nts_cig_depth_seg));
    host_segs = (nts_cig_depth_seg*)malloc(n_segs * sizeof(nts_cig_depth_seg));
    if (!host_segs) return fail(ctx, NTS_ENOMEM, "nts_cigar_depth: no host memory for the segments");
    {
      ScopedTimer t(ctx, "cigar_depth_emit", true);
      NTS_LAUNCH(k_cigd_emit, IVL_GRID(n_b), (const uint64_t*)d_bkey, (const uint64_t*)d_state, n_b, (const uint64_t*)d_rank, (const uint64_t*)d_r0, n_groups,
                 d_segs, n_segs);
    }
    e_run = hipGetLastError();
    if (e_run == hipSuccess) e_run = hipMemcpyAsync(host_segs, d_segs, n_segs * sizeof(nts_cig_depth_seg), hipMemcpyDeviceToHost, ctx->stream);
    e_sync = hipStreamSynchronize(ctx->stream);
    if (e_run != hipSuccess || e_sync != hipSuccess) free(host_segs);
    HIP_TRY(ctx, e_run);
    HIP_TRY(ctx, e_sync);
  }
  *segs = host_segs;
  memcpy(seg_first, host_seg_first.data(), (n_groups + 1) * 8);
  return NTS_OK;
}

// ---- variant sites over a star alignment: the bases at the X, D and I columns, and one allele table per group ----
// ---- (nts_cigar_var_bases, nts_cigar_alleles; ntsynt_amd/assess.py block_variant_sites) ----
// docs/design/04_32_block_variant_sites.md.  Both calls stage ONE functor, CigVarOf: (A bases, B bases, events, ref bytes, alt bytes)
// per entry -- an X of length L has L events, L ref bytes and L alt bytes; a D one event and L ref bytes; an I one event and L alt bytes.
// nts_cigar_var_bases (entries, records, spans, both genomes; nts_cigar_rows' checks): the REF bytes of a chain are row A at the columns
// of its X and D entries, the ALT bytes row B at those of its X and I entries.
//   1  the stage; k_cig_rows_firsts reads the ref and the alt prefix at every chain's first entry (timer "cigar_var_bases_scan").
//   2  k_cigv_bases: one lane per aligned 4-byte word of EITHER buffer (the ref words first); an upper-bound search over that buffer's
//      byte prefix finds the entry of the word's first byte, the lane walks on over the entries the word touches (entries without a
//      byte on its side are stepped over), composes four bytes through cig_rows_base and stores one dword (timer "cigar_var_bases_emit").
// nts_cigar_alleles (entries, records, {group, t0}, the alt bytes; nts_cigar_pad's checks; no genome): an EVENT is an X column (SNV), a D
// entry (DEL) or an I entry (INS); events with equal (group, pos, kind, len, alt bytes) are one ALLELE, its CARRIERS their chains.
//   1  the stage.  k_cigv_events: one lane per event -- its entry by an upper-bound search over the event prefix, its chain by one over
//      the chains' firsts -- stores key1 = group << 32 | pos - R0, key2 = kind << 62 | (the alt byte of an SNV, else len), its chain and
//      its two byte offsets.  Stable radix sort by key2 (the values: the event indices), key1 gathered in that order, stable radix sort
//      by key1, key2 gathered in the final order: events ascend by (key1, key2, event), so by chain inside a run (timer
//      "cigar_alleles_events").
//   2  k_cigv_leaders: one lane per sorted event; a lower-bound search gives the start of its run of equal (key1, key2); the leader of
//      an SNV or DEL is the run's start, of an INS the first event of the run with the same `len` alt bytes (cigv_same_bytes: dwords
//      where both offsets are congruent modulo 4) -- THE ONE NON-LINEAR STEP: an INS run of r events costs up to r (r - 1) / 2
//      comparisons of up to len bytes.  Stable radix sort of (leader, sorted index) -- it permutes inside runs only, so the sorted keys
//      stay valid by position --, a head flag per event, ONE exclusive scan, k_cigd_firsts for allele_first, and k_cigv_emit: a head
//      writes its allele but n_carriers, the last event of an allele n_carriers, every event its chain (timer "cigar_alleles_emit").
// No atomic, no floating point, no runtime division, no launch per chain, group, event or allele, no host loop over entries or events.

static_assert(sizeof(nts_cig_allele) == 56, "the C ABI's layout");
static_assert(NTS_OP_SUB == 1u && NTS_OP_DEL == 2u && NTS_OP_INS == 3u, "the kinds fit the two top bits of key2");

constexpr uint64_t CIGV_MOST_BYTES = 0xFFFFFFFFull;        // a buffer of nts_cigar_var_bases, and the events of nts_cigar_alleles, stay below 2^32
constexpr uint64_t CIGV_LEN = (1ull << 62) - 1u;           // key2's low bits (lengths are below 2^62: cig_chains_check)

using CigVarTuple = rocprim::tuple<uint64_t, uint64_t, uint64_t, uint64_t, uint64_t>; // A bases, B bases, events, ref bytes, alt bytes

struct CigVarOf // element e of the scan's input: what entry e consumes, its events and its bytes in either buffer; nothing behind the last entry
{
  using Tuple = CigVarTuple;
  const uint64_t* cigar;
  uint64_t n_cigar;
  __device__ Tuple operator()(uint64_t e) const
  {
    if (e >= n_cigar) return Tuple(0, 0, 0, 0, 0);
    const uint64_t v = cigar[e], code = v & 15u, len = v >> 4;
    const CigBases ab = cig_bases(v);
    const bool x = code == CIG_X, d = code == CIG_D, i = code == CIG_I;
    return Tuple(rocprim::get<0>(ab), rocprim::get<1>(ab), x ? len : (d || i ? 1u : 0u), x || d ? len : 0, x || i ? len : 0); // (each <= A + B bases: no wrap)
  }
};

// lane w < words_ref: word w of the ref bytes; lane words_ref + w, w < words_alt: word w of the alt bytes
__global__ __launch_bounds__(256) void k_cigv_bases(const uint64_t* __restrict__ cigar, uint64_t n_cigar, const CigTextChain* __restrict__ chains,
                                                    uint64_t n_chains, const uint64_t* __restrict__ PA, const uint64_t* __restrict__ PB,
                                                    const uint64_t* __restrict__ PR, const uint64_t* __restrict__ PL,
                                                    const uint8_t* __restrict__ code_a, uint64_t size_a, const uint8_t* __restrict__ code_b,
                                                    uint64_t size_b, uint32_t* __restrict__ out_ref, uint64_t words_ref, uint32_t* __restrict__ out_alt,
                                                    uint64_t words_alt)
{
  const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (g >= words_ref + words_alt || n_cigar == 0 || n_chains == 0) return;
  const bool is_alt = g >= words_ref;
  const uint64_t* __restrict__ P = is_alt ? PL : PR;
  const uint64_t w = is_alt ? g - words_ref : g, total = P[n_cigar], o = 4u * w;
  uint64_t e = cig_last_at_or_before(n_cigar, o, [P](uint64_t i) { return P[i]; }); // the entry of the word's first byte (P[0] = 0 <= o)
  uint64_t p0 = P[e], p1 = P[e + 1u]; // (e < n_cigar)
  uint64_t chain_of = ~0ull;
  CigTextChain ch = {};
  uint64_t in_a = 0, in_b = 0;
  uint32_t word = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    const uint64_t at = o + k;
    if (at >= total) break;                // (the padding of the last word stays 0)
    while (at >= p1 && e + 1u < n_cigar) { // the next entry with a byte on this side: entries without one have p1 = p0
      ++e;
      p0 = p1;
      p1 = P[e + 1u];
    }
    if (chain_of != e) {
      ch = chains[cig_last_at_or_before(n_chains, e, [chains](uint64_t c) { return chains[c].first; })];
      chain_of = e;
      const uint64_t f = ch.first <= e ? ch.first : e;
      in_a = PA[e] - PA[f];
      in_b = PB[e] - PB[f];
    }
    uint32_t byte = '?'; // (never seen: at < total lies inside an entry)
    if (at >= p0 && at < p1)
      byte = is_alt ? cig_rows_base(code_b, size_b, ch.at_b, in_b + (at - p0), ch.len_b, (ch.flags & NTS_CIG_B_BACKWARDS) != 0)
                    : cig_rows_base(code_a, size_a, ch.at_a, in_a + (at - p0), ch.len_a, false);
    word |= byte << (8u * k);
  }
  if (is_alt) out_alt[w] = word; // (w < words_alt)
  else out_ref[w] = word;
}

int cigar_var_bases_run(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains, const nts_genome* a,
                        const nts_genome* b, const nts_cig_span* spans, uint8_t** ref, uint64_t* ref_first, uint8_t** alt, uint64_t* alt_first)
{
  const char* const name = "nts_cigar_var_bases";
  std::vector<CigTextChain> placed(n_chains);
  auto place = [&](uint64_t c, auto who) -> int { return cig_rows_place(ctx, chains[c], spans[c], a, b, who, placed[c]); };
  if (const int rc = cig_chains_check(ctx, name, CIG_TEXT_MAX_BASES_LOG2, true, chains, n_chains, n_cigar, place)) return rc;
  auto nothing = [&] {
    *ref = nullptr;
    *alt = nullptr;
    memset(ref_first, 0, (n_chains + 1) * 8);
    memset(alt_first, 0, (n_chains + 1) * 8);
    return NTS_OK;
  };
  if (n_cigar == 0) return nothing(); // (nothing is launched)
  // (its own buffers first: while nothing is queued, a request that fails may still return at once)
  NTS_WS(d_placed, CigTextChain*, "cigv_placed", n_chains * sizeof(CigTextChain));
  NTS_WS(d_first, uint64_t*, "cigv_first", 2 * (n_chains + 1) * 8);
  std::vector<uint64_t> host_first(2 * (n_chains + 1)); // (the caller's arrays are written only when the call succeeds)
  uint32_t worst = SCRIPT_OK;
  CigIndex ix; // columns PA, PB, PE (events: not read here), PR (ref bytes), PL (alt bytes)
  hipError_t e_run;
  auto firsts = [&] {
    NTS_LAUNCH(k_cig_rows_firsts, IVL_GRID(n_chains + 1), ix.chains, n_chains, n_cigar, ix.column(3), d_first);
    NTS_LAUNCH(k_cig_rows_firsts, IVL_GRID(n_chains + 1), ix.chains, n_chains, n_cigar, ix.column(4), d_first + (n_chains + 1));
  };
  if (const int rc = cig_index_stage<CigVarOf>(ctx, "cigar_var_bases_scan", cigar, n_cigar, chains, n_chains, 0, &worst, ix, e_run, firsts)) return rc;
  if (e_run == hipSuccess) e_run = hipGetLastError();
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(d_placed, placed.data(), n_chains * sizeof(CigTextChain), hipMemcpyHostToDevice, ctx->stream);
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(host_first.data(), d_first, 2 * (n_chains + 1) * 8, hipMemcpyDeviceToHost, ctx->stream);
  hipError_t e_sync = hipStreamSynchronize(ctx->stream); // (whatever happened: the caller's arrays were sources of asynchronous copies)
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  if (worst != SCRIPT_OK) return fail(ctx, NTS_EINVAL, std::string(name) + ": the entries of chain " + std::to_string(worst) + " are no CIGAR of its lengths");
  const uint64_t n_ref = host_first[n_chains], n_alt = host_first[2 * n_chains + 1];
  if (n_ref > CIGV_MOST_BYTES || n_alt > CIGV_MOST_BYTES) return fail(ctx, NTS_ERANGE, std::string(name) + ": ref or alt bytes of 2^32 or more");
  if (n_ref + n_alt == 0) return nothing(); // (no chain with an X, D or I entry: no emit launch)
  const uint64_t words_ref = (n_ref + 3) / 4, words_alt = (n_alt + 3) / 4; // (the device buffers are padded to whole words)
  // (the stream is idle: the buffers are fetched before their kernel is queued)
  NTS_WS(d_ref, uint32_t*, "cigv_ref", std::max<uint64_t>(words_ref, 1) * 4);
  NTS_WS(d_alt, uint32_t*, "cigv_alt", std::max<uint64_t>(words_alt, 1) * 4);
  uint8_t* host_ref = n_ref ? (uint8_t*)malloc(n_ref) : nullptr;
  uint8_t* host_alt = n_alt ? (uint8_t*)malloc(n_alt) : nullptr;
  if ((n_ref && !host_ref) || (n_alt && !host_alt)) {
    free(host_ref);
    free(host_alt);
    return fail(ctx, NTS_ENOMEM, std::string(name) + ": no host memory for the bytes");
  }
  {
    ScopedTimer t(ctx, "cigar_var_bases_emit", true);
    NTS_LAUNCH(k_cigv_bases, IVL_GRID(words_ref + words_alt), ix.cigar, n_cigar, (const CigTextChain*)d_placed, n_chains, ix.column(0), ix.column(1),
               ix.column(3), ix.column(4), (const uint8_t*)a->d_code, a->n + 2 * PAD, (const uint8_t*)b->d_code, b->n + 2 * PAD, d_ref, words_ref, d_alt,
               words_alt);
  }
  e_run = hipGetLastError();
  if (e_run == hipSuccess && n_ref) e_run = hipMemcpyAsync(host_ref, d_ref, n_ref, hipMemcpyDeviceToHost, ctx->stream);
  if (e_run == hipSuccess && n_alt) e_run = hipMemcpyAsync(host_alt, d_alt, n_alt, hipMemcpyDeviceToHost, ctx->stream);
  e_sync = hipStreamSynchronize(ctx->stream);
  if (e_run != hipSuccess || e_sync != hipSuccess) {
    free(host_ref);
    free(host_alt);
  }
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  *ref = host_ref;
  *alt = host_alt;
  memcpy(ref_first, host_first.data(), (n_chains + 1) * 8);
  memcpy(alt_first, host_first.data() + (n_chains + 1), (n_chains + 1) * 8);
  return NTS_OK;
}

// lane i < n_ev: event i, in entry order (so in chain order)
__global__ __launch_bounds__(256) void k_cigv_events(const uint64_t* __restrict__ cigar, uint64_t n_cigar, const CigPadChain* __restrict__ placed,
                                                     uint64_t n_chains, const uint64_t* __restrict__ PA, const uint64_t* __restrict__ PE,
                                                     const uint64_t* __restrict__ PR, const uint64_t* __restrict__ PL, const uint8_t* __restrict__ alt,
                                                     uint64_t n_alt, uint64_t n_ev, uint64_t* __restrict__ key1, uint64_t* __restrict__ key2,
                                                     uint64_t* __restrict__ roff, uint64_t* __restrict__ aoff, uint32_t* __restrict__ chain)
{
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n_ev || n_cigar == 0 || n_chains == 0) return;
  const uint64_t e = cig_last_at_or_before(n_cigar, i, [PE](uint64_t k) { return PE[k]; }); // (PE[0] = 0 <= i < PE[n_cigar]: an entry with an event)
  const uint64_t c = cig_last_at_or_before(n_chains, e, [placed](uint64_t k) { return placed[k].first; });
  const CigPadChain ch = placed[c];
  const uint64_t f = ch.first <= e ? ch.first : e;
  const uint64_t v = cigar[e], code = v & 15u, len = v >> 4;
  const uint64_t off = code == CIG_X ? i - PE[e] : 0; // the column of an X entry
  uint64_t kind = NTS_OP_SUB, what = 0, r = PR[e] + off, l = PL[e] + off;
  if (code == CIG_X) {
    what = l < n_alt ? alt[l] : 0;
  } else if (code == CIG_D) {
    kind = NTS_OP_DEL;
    what = len & CIGV_LEN;
    l = 0;
  } else { // (CIG_I: = entries have no event)
    kind = NTS_OP_INS;
    what = len & CIGV_LEN;
    r = 0;
  }
  key1[i] = ch.key0 + (PA[e] - PA[f]) + off; // (n_ev words each)
  key2[i] = kind << 62 | what;
  roff[i] = r;
  aoff[i] = l;
  chain[i] = (uint32_t)c;
}

// lane j < n: dst[j] = src[at[j]] (at[j] < n, re-checked)
__global__ __launch_bounds__(256) void k_cigv_gather(const uint64_t* __restrict__ src, const uint64_t* __restrict__ at, uint64_t n, uint64_t* __restrict__ dst)
{
  const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (j >= n) return;
  const uint64_t i = at[j];
  dst[j] = i < n ? src[i] : 0;
}

// whether alt[a, a + len) and alt[b, b + len) are equal bytes (both inside n_alt: the caller's check)
__device__ __forceinline__ bool cigv_same_bytes(const uint8_t* __restrict__ alt, uint64_t a, uint64_t b, uint64_t len)
{
  uint64_t k = 0;
  if (((a ^ b) & 3u) == 0) { // congruent offsets: the aligned middle by dwords (the buffer begins at a multiple of 4)
    for (; k < len && ((a + k) & 3u) != 0; ++k)
      if (alt[a + k] != alt[b + k]) return false;
    for (; k + 4u <= len; k += 4u)
      if (*(const uint32_t*)(alt + a + k) != *(const uint32_t*)(alt + b + k)) return false;
  }
  for (; k < len; ++k)
    if (alt[a + k] != alt[b + k]) return false;
  return true;
}

// the first s < n with (key1[s], key2[s]) >= (k1, k2) over ascending pairs
__device__ __forceinline__ uint64_t cigv_lower(const uint64_t* __restrict__ key1, const uint64_t* __restrict__ key2, uint64_t n, uint64_t k1, uint64_t k2)
{
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2u;
    const uint64_t m1 = key1[mid];
    if (m1 < k1 || (m1 == k1 && key2[mid] < k2)) lo = mid + 1u;
    else hi = mid;
  }
  return lo;
}

// lane s < n_ev: the sorted index of the leader of sorted event s
__global__ __launch_bounds__(256) void k_cigv_leaders(const uint64_t* __restrict__ key1s, const uint64_t* __restrict__ key2s, const uint64_t* __restrict__ perm,
                                                      const uint64_t* __restrict__ aoff, const uint8_t* __restrict__ alt, uint64_t n_alt, uint64_t n_ev,
                                                      uint64_t* __restrict__ lead)
{
  const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (s >= n_ev) return;
  const uint64_t k1 = key1s[s], k2 = key2s[s];
  uint64_t start = cigv_lower(key1s, key2s, n_ev, k1, k2);
  if (start > s) start = s; // (ascending pairs: never)
  uint64_t say = start;
  if ((k2 >> 62) == NTS_OP_INS) {
    say = s;
    const uint64_t len = k2 & CIGV_LEN, i = perm[s], mine = i < n_ev ? aoff[i] : n_alt;
    if (mine <= n_alt && len <= n_alt - mine) {
      for (uint64_t j = start; j < s; ++j) { // the divergent loop: up to s - start comparisons of up to len bytes
        const uint64_t q = perm[j], theirs = q < n_ev ? aoff[q] : n_alt;
        if (theirs <= n_alt && len <= n_alt - theirs && cigv_same_bytes(alt, theirs, mine, len)) {
          say = j;
          break;
        }
      }
    }
  }
  lead[s] = say;
}

// lane t < n_ev: 1 where the event at t of the leader order opens an allele; lane n_ev: 0
__global__ __launch_bounds__(256) void k_cigv_heads(const uint64_t* __restrict__ leadc, uint64_t n_ev, uint64_t* __restrict__ head)
{
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t > n_ev) return;
  head[t] = t < n_ev && (t == 0 || leadc[t] != leadc[t - 1u]) ? 1u : 0u; // (n_ev + 1 words)
}

// lane t < n_ev: the event at t of the leader order; key1s and key2s hold by position (the leader sort permutes inside runs only)
__global__ __launch_bounds__(256) void k_cigv_emit(const uint64_t* __restrict__ key1s, const uint64_t* __restrict__ key2s, const uint64_t* __restrict__ perm,
                                                   const uint64_t* __restrict__ order, const uint64_t* __restrict__ leadc, const uint64_t* __restrict__ rank,
                                                   const uint64_t* __restrict__ roff, const uint64_t* __restrict__ aoff, const uint32_t* __restrict__ chain,
                                                   const uint64_t* __restrict__ r0, uint64_t n_groups, uint64_t n_ev, nts_cig_allele* __restrict__ alleles,
                                                   uint64_t n_alleles, uint32_t* __restrict__ carriers)
{
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= n_ev) return;
  const uint64_t s = order[t], i = s < n_ev ? perm[s] : n_ev;
  carriers[t] = i < n_ev ? chain[i] : 0xFFFFFFFFu; // (n_ev words)
  const uint64_t r = rank[t + 1u] - 1u;             // the heads up to and with t, less one (rank: n_ev + 1 words; 0 - 1: beyond n_alleles)
  if (r >= n_alleles || i >= n_ev) return;
  const uint64_t me = leadc[t];
  if (t == 0 || leadc[t - 1u] != me) { // a head: its event is the leader
    const uint64_t k1 = key1s[t], k2 = key2s[t], group = k1 >> 32, kind = k2 >> 62;
    alleles[r].pos = (group < n_groups ? r0[group] : 0) + (k1 & 0xFFFFFFFFull);
    alleles[r].len = kind == NTS_OP_SUB ? 1u : k2 & CIGV_LEN;
    alleles[r].ref_off = roff[i];
    alleles[r].alt_off = aoff[i];
    alleles[r].carrier_first = t;
    alleles[r].group = (uint32_t)group;
    alleles[r].kind = (uint32_t)kind;
    alleles[r].reserved = 0;
  }
  if (t + 1u == n_ev || leadc[t + 1u] != me) alleles[r].n_carriers = (uint32_t)(t + 1u - cigp_lower(leadc, n_ev, me)); // the last event of the allele
}

// the temporary of the sorts and the scan that nts_cigar_alleles and nts_cigar_profile queue behind the stage: the shared "ivs_tmp",
// fetched a second time per docs/design/04_24_call_order.md's rule, once every size is known
inline void* cigv_sort_tmp(nts_ctx* ctx, size_t bytes)
{
  return ws_get(ctx, "ivs_tmp", std::max<size_t>(bytes, 16));
}

// nts_cigar_pad's checks of chain c and its place: group order and range, a core, t0 + len_a, the extent of its group; r0[group] = the
// smallest t0 of the group so far, placed = {first, t0} (the key once every chain of the group is seen: cigv_keys)
template <class Who>
int cigv_place(nts_ctx* ctx, const uint64_t* cigar, const nts_cig_chain* chains, const nts_cig_pad_at* at, uint64_t n_groups, uint64_t c, Who who,
               uint64_t& lo, uint64_t& hi, std::vector<uint64_t>& r0, CigPadChain& placed)
{
  const nts_cig_chain& ch = chains[c];
  const nts_cig_pad_at& a = at[c];
  if (a.group >= n_groups) return fail(ctx, NTS_EINVAL, who() + " names a group outside n_groups");
  if (c && a.group < at[c - 1].group) return fail(ctx, NTS_EINVAL, who() + ": the groups are not nondecreasing");
  if (ch.n_cig) {
    const uint64_t head = cigar[ch.first] & 15u, tail = cigar[ch.first + ch.n_cig - 1u] & 15u;
    if ((head != CIG_EQ && head != CIG_X) || (tail != CIG_EQ && tail != CIG_X))
      return fail(ctx, NTS_EINVAL, who() + ": its first or last entry is not = or X (pass the core of a chain)");
  }
  if (a.t0 > ~0ull - ch.len_a) return fail(ctx, NTS_ERANGE, who() + ": t0 + len_a wraps");
  const bool opens = c == 0 || a.group != at[c - 1].group;
  lo = opens ? a.t0 : std::min(lo, a.t0);
  hi = opens ? a.t0 + ch.len_a : std::max(hi, a.t0 + ch.len_a);
  if (hi - lo > 0xFFFFFFFFull) return fail(ctx, NTS_ERANGE, who() + ": the reference extent of its group is 2^32 or more");
  r0[a.group] = lo;
  placed = { ch.first, a.t0 };
  return NTS_OK;
}

int cigar_alleles_run(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains, const nts_cig_pad_at* at,
                      uint64_t n_groups, const uint8_t* alt, uint64_t n_alt, nts_cig_allele** alleles, uint64_t* allele_first, uint32_t** carriers,
                      uint64_t* n_carriers)
{
  std::vector<CigPadChain> placed;
  std::vector<uint64_t> r0;
  try {
    placed.resize(n_chains);
    r0.assign(std::max<uint64_t>(n_groups, 1), 0);
  } catch (const std::bad_alloc&) {
    return fail(ctx, NTS_ENOMEM, "nts_cigar_alleles: no host memory for the chains and groups");
  }
  uint64_t lo = 0, hi = 0; // the extent of the group of the chain in front
  auto place = [&](uint64_t c, auto who) -> int { return cigv_place(ctx, cigar, chains, at, n_groups, c, who, lo, hi, r0, placed[c]); };
  if (const int rc = cig_chains_check(ctx, "nts_cigar_alleles", CIG_TEXT_MAX_BASES_LOG2, true, chains, n_chains, n_cigar, place)) return rc;
  for (uint64_t c = 0; c < n_chains; ++c) placed[c].key0 = ((uint64_t)at[c].group << 32) + (placed[c].key0 - r0[at[c].group]);
  auto nothing = [&] {
    *alleles = nullptr;
    *carriers = nullptr;
    *n_carriers = 0;
    memset(allele_first, 0, (n_groups + 1) * 8);
    return NTS_OK;
  };
  if (n_cigar == 0) { // (nothing is launched)
    if (n_alt) return fail(ctx, NTS_EINVAL, "nts_cigar_alleles: alt holds " + std::to_string(n_alt) + " bytes, the X and I entries of the chains have 0");
    return nothing();
  }
  // (its own buffers first: while nothing is queued, a request that fails may still return at once)
  NTS_WS(d_placed, CigPadChain*, "cigv_placed_at", n_chains * sizeof(CigPadChain));
  NTS_WS(d_r0, uint64_t*, "cigv_r0", std::max<uint64_t>(n_groups, 1) * 8);
  NTS_WS(d_allele_first, uint64_t*, "cigv_allele_first", (n_groups + 2) * 8);
  uint32_t worst = SCRIPT_OK;
  uint64_t totals[3] = { 0, 0, 0 }; // events, ref bytes, alt bytes
  CigIndex ix; // columns PA, PB, PE (events), PR (ref bytes), PL (alt bytes)
  hipError_t e_run;
  if (const int rc = cig_index_stage<CigVarOf>(ctx, "cigar_alleles_events", cigar, n_cigar, chains, n_chains, 0, &worst, ix, e_run, [] {})) return rc;
  if (e_run == hipSuccess) e_run = hipGetLastError();
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(d_placed, placed.data(), n_chains * sizeof(CigPadChain), hipMemcpyHostToDevice, ctx->stream);
  if (e_run == hipSuccess && n_groups) e_run = hipMemcpyAsync(d_r0, r0.data(), n_groups * 8, hipMemcpyHostToDevice, ctx->stream);
  for (uint32_t k = 0; k < 3 && e_run == hipSuccess; ++k)
    e_run = hipMemcpyAsync(&totals[k], ix.column(2 + k) + n_cigar, 8, hipMemcpyDeviceToHost, ctx->stream);
  hipError_t e_sync = hipStreamSynchronize(ctx->stream); // (whatever happened: the caller's arrays were sources of asynchronous copies)
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  if (worst != SCRIPT_OK) {
    if (worst < n_chains) // (the error path alone looks at the entries of that one chain)
      for (uint64_t e = chains[worst].first; e < chains[worst].first + chains[worst].n_cig; ++e)
        if ((cigar[e] & 15u) == CIG_P) return fail(ctx, NTS_EINVAL, "nts_cigar_alleles: chain " + std::to_string(worst) + " holds an entry of code 6");
    return fail(ctx, NTS_EINVAL, "nts_cigar_alleles: the entries of chain " + std::to_string(worst) + " are no CIGAR of its lengths");
  }
  const uint64_t n_ev = totals[0];
  if (totals[2] != n_alt)
    return fail(ctx, NTS_EINVAL, "nts_cigar_alleles: alt holds " + std::to_string(n_alt) + " bytes, the X and I entries of the chains have " + std::to_string(totals[2]));
  if (n_ev > CIGV_MOST_BYTES) return fail(ctx, NTS_ERANGE, "nts_cigar_alleles: 2^32 events or more");
  if (n_ev == 0) return nothing(); // (no launch behind the stage)
  // (the stream is idle: the buffers sized by the events are fetched before their kernels are queued)
  NTS_WS(d_alt, uint8_t*, "cigv_alt_in", (std::max<uint64_t>(n_alt, 1) + 3) / 4 * 4);
  NTS_WS(d_key1, uint64_t*, "cigv_key1", n_ev * 8);
  NTS_WS(d_key2, uint64_t*, "cigv_key2", n_ev * 8);
  NTS_WS(d_roff, uint64_t*, "cigv_roff", n_ev * 8);
  NTS_WS(d_aoff, uint64_t*, "cigv_aoff", n_ev * 8);
  NTS_WS(d_chain, uint32_t*, "cigv_chain", n_ev * 4);
  NTS_WS(d_key2a, uint64_t*, "cigv_key2a", n_ev * 8);
  NTS_WS(d_idxa, uint64_t*, "cigv_idxa", n_ev * 8);
  NTS_WS(d_key1a, uint64_t*, "cigv_key1a", n_ev * 8);
  NTS_WS(d_key1s, uint64_t*, "cigv_key1s", n_ev * 8);
  NTS_WS(d_perm, uint64_t*, "cigv_perm", n_ev * 8);
  NTS_WS(d_key2s, uint64_t*, "cigv_key2s", n_ev * 8);
  NTS_WS(d_lead, uint64_t*, "cigv_lead", n_ev * 8);
  NTS_WS(d_leadc, uint64_t*, "cigv_leadc", n_ev * 8);
  NTS_WS(d_order, uint64_t*, "cigv_order", n_ev * 8);
  NTS_WS(d_head, uint64_t*, "cigv_head", (n_ev + 1) * 8);
  NTS_WS(d_rank, uint64_t*, "cigv_rank", (n_ev + 1) * 8);
  NTS_WS(d_carriers, uint32_t*, "cigv_carriers", n_ev * 4);
  const rocprim::counting_iterator<uint64_t> iota(0);
  size_t tmp_a = 0, tmp_b = 0, tmp_c = 0, tmp_scan = 0;
  e_run = rocprim::radix_sort_pairs(nullptr, tmp_a, d_key2, d_key2a, iota, d_idxa, n_ev, 0, 64, ctx->stream);
  if (e_run == hipSuccess) e_run = rocprim::radix_sort_pairs(nullptr, tmp_b, d_key1a, d_key1s, d_idxa, d_perm, n_ev, 0, 64, ctx->stream);
  if (e_run == hipSuccess) e_run = rocprim::radix_sort_pairs(nullptr, tmp_c, d_lead, d_leadc, iota, d_order, n_ev, 0, 32, ctx->stream);
  if (e_run == hipSuccess) e_run = rocprim::exclusive_scan(nullptr, tmp_scan, d_head, d_rank, (uint64_t)0, n_ev + 1, rocprim::plus<uint64_t>(), ctx->stream);
  HIP_TRY(ctx, e_run);
  void* const d_tmp = cigv_sort_tmp(ctx, std::max(std::max(tmp_a, tmp_b), std::max(tmp_c, tmp_scan))); // (ix.tmp is dead from here)
  if (!d_tmp) return NTS_ENOMEM;
  std::vector<uint64_t> host_first(n_groups + 2); // (the caller's array is written only when the call succeeds)
  if (n_alt) e_run = hipMemcpyAsync(d_alt, alt, n_alt, hipMemcpyHostToDevice, ctx->stream); // (a source of an asynchronous copy: a synchronisation follows whatever happens)
  if (e_run == hipSuccess) {
    ScopedTimer t(ctx, "cigar_alleles_events", true);
    NTS_LAUNCH(k_cigv_events, IVL_GRID(n_ev), ix.cigar, n_cigar, (const CigPadChain*)d_placed, n_chains, ix.column(0), ix.column(2), ix.column(3),
               ix.column(4), (const uint8_t*)d_alt, n_alt, n_ev, d_key1, d_key2, d_roff, d_aoff, d_chain);
    e_run = rocprim::radix_sort_pairs(d_tmp, tmp_a, d_key2, d_key2a, iota, d_idxa, n_ev, 0, 64, ctx->stream);
    if (e_run == hipSuccess) {
      NTS_LAUNCH(k_cigv_gather, IVL_GRID(n_ev), (const uint64_t*)d_key1, (const uint64_t*)d_idxa, n_ev, d_key1a);
      e_run = rocprim::radix_sort_pairs(d_tmp, tmp_b, d_key1a, d_key1s, d_idxa, d_perm, n_ev, 0, 64, ctx->stream);
    }
    if (e_run == hipSuccess) NTS_LAUNCH(k_cigv_gather, IVL_GRID(n_ev), (const uint64_t*)d_key2, (const uint64_t*)d_perm, n_ev, d_key2s);
  }
  if (e_run == hipSuccess) {
    ScopedTimer t(ctx, "cigar_alleles_emit", true);
    NTS_LAUNCH(k_cigv_leaders, IVL_GRID(n_ev), (const uint64_t*)d_key1s, (const uint64_t*)d_key2s, (const uint64_t*)d_perm, (const uint64_t*)d_aoff,
               (const uint8_t*)d_alt, n_alt, n_ev, d_lead);
    e_run = rocprim::radix_sort_pairs(d_tmp, tmp_c, d_lead, d_leadc, iota, d_order, n_ev, 0, 32, ctx->stream); // (a leader is a sorted index below 2^32)
    if (e_run == hipSuccess) {
      NTS_LAUNCH(k_cigv_heads, IVL_GRID(n_ev + 1), (const uint64_t*)d_leadc, n_ev, d_head);
      e_run = rocprim::exclusive_scan(d_tmp, tmp_scan, d_head, d_rank, (uint64_t)0, n_ev + 1, rocprim::plus<uint64_t>(), ctx->stream);
    }
    if (e_run == hipSuccess)
      NTS_LAUNCH(k_cigd_firsts, IVL_GRID(n_groups + 2), (const uint64_t*)d_key1s, n_ev, (const uint64_t*)d_rank, n_groups, d_allele_first);
  }
  if (e_run == hipSuccess) e_run = hipGetLastError();
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(host_first.data(), d_allele_first, (n_groups + 2) * 8, hipMemcpyDeviceToHost, ctx->stream);
  e_sync = hipStreamSynchronize(ctx->stream);
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  const uint64_t n_alleles = host_first[n_groups];
  if (n_alleles == 0 || n_alleles > n_ev) return fail(ctx, NTS_EHIP, "nts_cigar_alleles: the scan left an impossible number of alleles");
  // (the stream is idle: the output's buffer is fetched before its kernel is queued)
  NTS_WS(d_alleles, nts_cig_allele*, "cigv_alleles", n_alleles * sizeof(nts_cig_allele));
  nts_cig_allele* host_alleles = (nts_cig_allele*)malloc(n_alleles * sizeof(nts_cig_allele));
  uint32_t* host_carriers = (uint32_t*)malloc(n_ev * 4);
  auto drop = [&] {
    free(host_alleles);
    free(host_carriers);
  };
  if (!host_alleles || !host_carriers) {
    drop();
    return fail(ctx, NTS_ENOMEM, "nts_cigar_alleles: no host memory for the alleles");
  }
  {
    ScopedTimer t(ctx, "cigar_alleles_emit", true);
    NTS_LAUNCH(k_cigv_emit, IVL_GRID(n_ev), (const uint64_t*)d_key1s, (const uint64_t*)d_key2s, (const uint64_t*)d_perm, (const uint64_t*)d_order,
               (const uint64_t*)d_leadc, (const uint64_t*)d_rank, (const uint64_t*)d_roff, (const uint64_t*)d_aoff, (const uint32_t*)d_chain,
               (const uint64_t*)d_r0, n_groups, n_ev, d_alleles, n_alleles, d_carriers);
  }
  e_run = hipGetLastError();
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(host_alleles, d_alleles, n_alleles * sizeof(nts_cig_allele), hipMemcpyDeviceToHost, ctx->stream);
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(host_carriers, d_carriers, n_ev * 4, hipMemcpyDeviceToHost, ctx->stream);
  e_sync = hipStreamSynchronize(ctx->stream);
  if (e_run != hipSuccess || e_sync != hipSuccess) drop();
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  *alleles = host_alleles;
  *carriers = host_carriers;
  *n_carriers = n_ev;
  memcpy(allele_first, host_first.data(), (n_groups + 1) * 8);
  return NTS_OK;
}

// ---- per-column profile and consensus over a star alignment (nts_cigar_profile; ntsynt_amd/assess.py block_consensus) ----
// docs/design/04_33_block_consensus.md.  The third reader of a group of chains: one record per VARIABLE column of the group's star
// alignment -- every reference base at which some covering chain has an X or a D, and every column of every insertion slot -- with how
// many chains cover it, how many hold each of A, C, G, T, N or a gap there, the reference's byte and the plurality call.
//   1  cig_index_stage with CigProfOf: (A bases, B bases, events, ref bytes, alt bytes), an X, D or I entry of length L having L events.
//      k_cigf_events: one lane per event -- its entry by an upper-bound search over the event prefix, its chain by one over the chains'
//      firsts -- stores key1 = group << 32 | pos - R0, key2 = sub << 3 | symbol (sub: the column inside an I entry, NTS_CIG_PROFILE_REF
//      for an X or D column; symbol: A C G T N 0..4, 5 a deleted base) and its ref byte's offset.  Stable radix sort by key2 (35 bits;
//      the values: the event indices), key1 gathered in that order, stable radix sort by key1, key2 gathered in the final order: events
//      ascend by (group, pos, sub, symbol, event), so by chain inside a run.  k_cigf_chain_keys: one lane per chain, group << 32 |
//      t0 - R0 and group << 32 | t1 - R0; two radix sorts of them (timer "cigar_profile_events").
//   2  k_cigf_heads: a flag where (group, pos, sub) changes; ONE exclusive scan; k_cigd_firsts for col_first; k_cigf_emit: one lane
//      per sorted event, a head alone goes on: six bounded lower-bound searches inside its column's run give the per-symbol counts,
//      two cigp_lower searches over the chains' sorted keys give aligned = (chains of the group with t0 <= pos) - (those with t1 <= pos),
//      match = aligned - gap - sum n, the ref byte is that of the column's smallest event (its smallest chain), the call is decided and
//      the whole 56-byte record is stored (timer "cigar_profile_emit").
// No atomic, no floating point, no runtime division, no launch per chain, group, site or column, no host loop over entries, events or
// columns (one over chains: the checks and R0).

static_assert(sizeof(nts_cig_profile_col) == 56, "the C ABI's layout");

constexpr uint64_t CIGF_SYMBOLS = 6;  // A C G T N and the gap
constexpr uint64_t CIGF_GAP = 5;
constexpr uint32_t CIGF_KEY2_BITS = 35; // sub << 3 | symbol

struct CigProfOf // element e of the scan's input: what entry e consumes, its events (one per column of an X, D or I) and its bytes; nothing behind the last entry
{
  using Tuple = CigVarTuple;
  const uint64_t* cigar;
  uint64_t n_cigar;
  __device__ Tuple operator()(uint64_t e) const
  {
    if (e >= n_cigar) return Tuple(0, 0, 0, 0, 0);
    const uint64_t v = cigar[e], code = v & 15u, len = v >> 4;
    const CigBases ab = cig_bases(v);
    const bool x = code == CIG_X, d = code == CIG_D, i = code == CIG_I;
    return Tuple(rocprim::get<0>(ab), rocprim::get<1>(ab), x || d || i ? len : 0, x || d ? len : 0, x || i ? len : 0); // (each <= A + B bases: no wrap)
  }
};

// A C G T -> 0..3, any other byte -> 4 (N)
__host__ __device__ inline uint32_t cigf_symbol(uint32_t byte)
{
  return byte == 'A' ? 0u : byte == 'C' ? 1u : byte == 'G' ? 2u : byte == 'T' ? 3u : 4u;
}

// lane i < n_ev: event i, in entry order (so in chain order)
__global__ __launch_bounds__(256) void k_cigf_events(const uint64_t* __restrict__ cigar, uint64_t n_cigar, const CigPadChain* __restrict__ placed,
                                                     uint64_t n_chains, const uint64_t* __restrict__ PA, const uint64_t* __restrict__ PE,
                                                     const uint64_t* __restrict__ PR, const uint64_t* __restrict__ PL, const uint8_t* __restrict__ alt,
                                                     uint64_t n_alt, uint64_t n_ev, uint64_t* __restrict__ key1, uint64_t* __restrict__ key2,
                                                     uint32_t* __restrict__ roff)
{
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n_ev || n_cigar == 0 || n_chains == 0) return;
  const uint64_t e = cig_last_at_or_before(n_cigar, i, [PE](uint64_t k) { return PE[k]; }); // (PE[0] = 0 <= i < PE[n_cigar]: an entry with an event)
  const uint64_t c = cig_last_at_or_before(n_chains, e, [placed](uint64_t k) { return placed[k].first; });
  const CigPadChain ch = placed[c];
  const uint64_t f = ch.first <= e ? ch.first : e;
  const uint64_t code = cigar[e] & 15u, off = i - PE[e]; // the column inside the entry (off < n_ev < 2^32)
  uint64_t at = ch.key0 + (PA[e] - PA[f]), sub = NTS_CIG_PROFILE_REF, symbol = CIGF_GAP, r = 0;
  if (code == CIG_I) {
    sub = off;
  } else { // (CIG_X or CIG_D: = entries have no event)
    at += off;
    r = PR[e] + off;
  }
  if (code != CIG_D) {
    const uint64_t l = PL[e] + off;
    symbol = cigf_symbol(l < n_alt ? alt[l] : 0);
  }
  key1[i] = at; // (n_ev words each)
  key2[i] = sub << 3 | symbol;
  roff[i] = (uint32_t)r; // (the ref bytes are as many as the X and D events: below 2^32)
}

// lane c < n_chains: the keys of where chain c begins and ends on its group's reference
__global__ __launch_bounds__(256) void k_cigf_chain_keys(const CigPadChain* __restrict__ placed, const nts_cig_chain* __restrict__ chains, uint64_t n_chains,
                                                         uint64_t* __restrict__ begins, uint64_t* __restrict__ ends)
{
  const uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (c >= n_chains) return;
  const uint64_t k = placed[c].key0;
  begins[c] = k;
  ends[c] = k + chains[c].len_a; // (t1 - R0 <= 2^32 - 1: the extent of a group was checked)
}

// lane t < n_ev: 1 where the sorted event at t opens a column; lane n_ev: 0
__global__ __launch_bounds__(256) void k_cigf_heads(const uint64_t* __restrict__ key1s, const uint64_t* __restrict__ key2s, uint64_t n_ev,
                                                    uint64_t* __restrict__ head)
{
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t > n_ev) return;
  head[t] = t < n_ev && (t == 0 || key1s[t] != key1s[t - 1u] || (key2s[t] >> 3) != (key2s[t - 1u] >> 3)) ? 1u : 0u; // (n_ev + 1 words)
}

// the first s in [lo, n) with (key1[s], key2[s]) >= (k1, k2) over ascending pairs
__device__ __forceinline__ uint64_t cigf_lower_from(const uint64_t* __restrict__ key1, const uint64_t* __restrict__ key2, uint64_t lo, uint64_t n, uint64_t k1,
                                                    uint64_t k2)
{
  uint64_t hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2u;
    const uint64_t m1 = key1[mid];
    if (m1 < k1 || (m1 == k1 && key2[mid] < k2)) lo = mid + 1u;
    else hi = mid;
  }
  return lo;
}

// lane t < n_ev: the sorted event at t; one that opens a column writes the column's whole record
__global__ __launch_bounds__(256) void k_cigf_emit(const uint64_t* __restrict__ key1s, const uint64_t* __restrict__ key2s, const uint64_t* __restrict__ perm,
                                                   const uint64_t* __restrict__ rank, const uint32_t* __restrict__ roff, const uint8_t* __restrict__ ref,
                                                   uint64_t n_ref, const uint64_t* __restrict__ begins, const uint64_t* __restrict__ ends, uint64_t n_chains,
                                                   const uint64_t* __restrict__ r0, uint64_t n_groups, uint64_t n_ev, nts_cig_profile_col* __restrict__ cols,
                                                   uint64_t n_cols)
{
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= n_ev) return;
  const uint64_t k1 = key1s[t], k2 = key2s[t], sub = k2 >> 3;
  if (t > 0 && key1s[t - 1u] == k1 && (key2s[t - 1u] >> 3) == sub) return; // no head
  const uint64_t r = rank[t]; // the heads in front of t (rank: n_ev + 1 words)
  if (r >= n_cols) return;
  const bool is_ref = sub == NTS_CIG_PROFILE_REF;
  // the runs of the six symbols inside the column: [b, next b)
  uint64_t b = t, first_ev = ~0ull, sum = 0;
  uint32_t count[CIGF_SYMBOLS];
#pragma unroll
  for (uint32_t s = 0; s < CIGF_SYMBOLS; ++s) {
    const uint64_t e = cigf_lower_from(key1s, key2s, b, n_ev, k1, (sub << 3) + s + 1u);
    if (e > b) { // the run's first event is that of its smallest chain
      const uint64_t i = perm[b];
      first_ev = i < first_ev ? i : first_ev;
    }
    count[s] = (uint32_t)(e - b);
    sum += e - b;
    b = e;
  }
  // the chains of the group that begin at or in front of pos, less those that end there or in front of it (equal keys: the same group's chains in front)
  const uint64_t aligned = cigp_lower(begins, n_chains, k1 + 1u) - cigp_lower(ends, n_chains, k1 + 1u);
  const uint64_t group = k1 >> 32;
  nts_cig_profile_col out;
  out.pos = (group < n_groups ? r0[group] : 0) + (k1 & 0xFFFFFFFFull);
  out.group = (uint32_t)group;
  out.sub = (uint32_t)sub;
  out.aligned = (uint32_t)aligned;
  uint32_t tally[CIGF_SYMBOLS], ref_symbol = CIGF_GAP;
#pragma unroll
  for (uint32_t s = 0; s < CIGF_SYMBOLS; ++s) tally[s] = count[s];
  if (is_ref) {
    const uint64_t at = first_ev < n_ev ? roff[first_ev] : n_ref;
    out.ref = at < n_ref ? ref[at] : (uint8_t)'N';
    out.gap = count[CIGF_GAP];
    out.match = (uint32_t)(aligned - sum);
    ref_symbol = cigf_symbol(out.ref);
#pragma unroll
    for (uint32_t s = 0; s < 5u; ++s) tally[s] += s == ref_symbol ? out.match + 1u : 0u; // the reference row and the chains that equal it
  } else {
    out.ref = (uint8_t)'-';
    out.gap = (uint32_t)(aligned - sum); // (an insertion column has no event of symbol 5)
    out.match = 0;
    tally[CIGF_GAP] = out.gap + 1u; // the reference row
  }
  uint32_t best = 0;
#pragma unroll
  for (uint32_t s = 1; s < CIGF_SYMBOLS; ++s) best = tally[s] > tally[best] ? s : best; // the first of A C G T N - among the largest
  uint32_t ref_tally = 0;
#pragma unroll
  for (uint32_t s = 0; s < CIGF_SYMBOLS; ++s) ref_tally = s == ref_symbol ? tally[s] : ref_tally;
  uint32_t most = 0;
#pragma unroll
  for (uint32_t s = 0; s < CIGF_SYMBOLS; ++s) most = s == best ? tally[s] : most;
  if (ref_tally == most) best = ref_symbol;
#pragma unroll
  for (uint32_t s = 0; s < 5u; ++s) out.n[s] = count[s];
  out.call = (uint8_t)(best == 0 ? 'A' : best == 1 ? 'C' : best == 2 ? 'G' : best == 3 ? 'T' : best == 4 ? 'N' : '-');
#pragma unroll
  for (uint32_t k = 0; k < 6u; ++k) out.reserved[k] = 0;
  cols[r] = out; // (every byte of the record, once)
}

int cigar_profile_run(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains, const nts_cig_pad_at* at,
                      uint64_t n_groups, const uint8_t* ref, uint64_t n_ref, const uint8_t* alt, uint64_t n_alt, nts_cig_profile_col** cols,
                      uint64_t* col_first)
{
  std::vector<CigPadChain> placed;
  std::vector<uint64_t> r0;
  try {
    placed.resize(n_chains);
    r0.assign(std::max<uint64_t>(n_groups, 1), 0);
  } catch (const std::bad_alloc&) {
    return fail(ctx, NTS_ENOMEM, "nts_cigar_profile: no host memory for the chains and groups");
  }
  uint64_t lo = 0, hi = 0; // the extent of the group of the chain in front
  auto place = [&](uint64_t c, auto who) -> int { return cigv_place(ctx, cigar, chains, at, n_groups, c, who, lo, hi, r0, placed[c]); };
  if (const int rc = cig_chains_check(ctx, "nts_cigar_profile", CIG_TEXT_MAX_BASES_LOG2, true, chains, n_chains, n_cigar, place)) return rc;
  for (uint64_t c = 0; c < n_chains; ++c) placed[c].key0 = ((uint64_t)at[c].group << 32) + (placed[c].key0 - r0[at[c].group]);
  auto nothing = [&] {
    *cols = nullptr;
    memset(col_first, 0, (n_groups + 1) * 8);
    return NTS_OK;
  };
  auto bytes_differ = [&](const char* which, uint64_t given, const char* entries, uint64_t have) {
    return fail(ctx, NTS_EINVAL, std::string("nts_cigar_profile: ") + which + " holds " + std::to_string(given) + " bytes, the " + entries +
                                   " entries of the chains have " + std::to_string(have));
  };
  if (n_cigar == 0) { // (nothing is launched)
    if (n_alt) return bytes_differ("alt", n_alt, "X and I", 0);
    if (n_ref) return bytes_differ("ref", n_ref, "X and D", 0);
    return nothing();
  }
  // (its own buffers first: while nothing is queued, a request that fails may still return at once)
  NTS_WS(d_placed, CigPadChain*, "cigf_placed", n_chains * sizeof(CigPadChain));
  NTS_WS(d_r0, uint64_t*, "cigf_r0", std::max<uint64_t>(n_groups, 1) * 8);
  NTS_WS(d_col_first, uint64_t*, "cigf_col_first", (n_groups + 2) * 8);
  NTS_WS(d_begins, uint64_t*, "cigf_begins", n_chains * 8);
  NTS_WS(d_ends, uint64_t*, "cigf_ends", n_chains * 8);
  NTS_WS(d_begins_s, uint64_t*, "cigf_begins_s", n_chains * 8);
  NTS_WS(d_ends_s, uint64_t*, "cigf_ends_s", n_chains * 8);
  uint32_t worst = SCRIPT_OK;
  uint64_t totals[3] = { 0, 0, 0 }; // events, ref bytes, alt bytes
  CigIndex ix; // columns PA, PB, PE (events), PR (ref bytes), PL (alt bytes)
  hipError_t e_run;
  if (const int rc = cig_index_stage<CigProfOf>(ctx, "cigar_profile_events", cigar, n_cigar, chains, n_chains, 0, &worst, ix, e_run, [] {})) return rc;
  if (e_run == hipSuccess) e_run = hipGetLastError();
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(d_placed, placed.data(), n_chains * sizeof(CigPadChain), hipMemcpyHostToDevice, ctx->stream);
  if (e_run == hipSuccess && n_groups) e_run = hipMemcpyAsync(d_r0, r0.data(), n_groups * 8, hipMemcpyHostToDevice, ctx->stream);
  for (uint32_t k = 0; k < 3 && e_run == hipSuccess; ++k)
    e_run = hipMemcpyAsync(&totals[k], ix.column(2 + k) + n_cigar, 8, hipMemcpyDeviceToHost, ctx->stream);
  hipError_t e_sync = hipStreamSynchronize(ctx->stream); // (whatever happened: the caller's arrays were sources of asynchronous copies)
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  if (worst != SCRIPT_OK) {
    if (worst < n_chains) // (the error path alone looks at the entries of that one chain)
      for (uint64_t e = chains[worst].first; e < chains[worst].first + chains[worst].n_cig; ++e)
        if ((cigar[e] & 15u) == CIG_P) return fail(ctx, NTS_EINVAL, "nts_cigar_profile: chain " + std::to_string(worst) + " holds an entry of code 6");
    return fail(ctx, NTS_EINVAL, "nts_cigar_profile: the entries of chain " + std::to_string(worst) + " are no CIGAR of its lengths");
  }
  const uint64_t n_ev = totals[0];
  if (totals[2] != n_alt) return bytes_differ("alt", n_alt, "X and I", totals[2]);
  if (totals[1] != n_ref) return bytes_differ("ref", n_ref, "X and D", totals[1]);
  if (n_ev > CIGV_MOST_BYTES) return fail(ctx, NTS_ERANGE, "nts_cigar_profile: 2^32 events or more");
  if (n_ev == 0) return nothing(); // (no launch behind the stage)
  // (the stream is idle: the buffers sized by the events are fetched before their kernels are queued)
  NTS_WS(d_alt, uint8_t*, "cigf_alt_in", (std::max<uint64_t>(n_alt, 1) + 3) / 4 * 4);
  NTS_WS(d_ref, uint8_t*, "cigf_ref_in", (std::max<uint64_t>(n_ref, 1) + 3) / 4 * 4);
  NTS_WS(d_key1, uint64_t*, "cigf_key1", n_ev * 8);
  NTS_WS(d_key2, uint64_t*, "cigf_key2", n_ev * 8);
  NTS_WS(d_roff, uint32_t*, "cigf_roff", n_ev * 4);
  NTS_WS(d_key2a, uint64_t*, "cigf_key2a", n_ev * 8);
  NTS_WS(d_idxa, uint64_t*, "cigf_idxa", n_ev * 8);
  NTS_WS(d_key1a, uint64_t*, "cigf_key1a", n_ev * 8);
  NTS_WS(d_key1s, uint64_t*, "cigf_key1s", n_ev * 8);
  NTS_WS(d_perm, uint64_t*, "cigf_perm", n_ev * 8);
  NTS_WS(d_key2s, uint64_t*, "cigf_key2s", n_ev * 8);
  NTS_WS(d_head, uint64_t*, "cigf_head", (n_ev + 1) * 8);
  NTS_WS(d_rank, uint64_t*, "cigf_rank", (n_ev + 1) * 8);
  const rocprim::counting_iterator<uint64_t> iota(0);
  size_t tmp_a = 0, tmp_b = 0, tmp_c = 0, tmp_scan = 0;
  e_run = rocprim::radix_sort_pairs(nullptr, tmp_a, d_key2, d_key2a, iota, d_idxa, n_ev, 0, CIGF_KEY2_BITS, ctx->stream);
  if (e_run == hipSuccess) e_run = rocprim::radix_sort_pairs(nullptr, tmp_b, d_key1a, d_key1s, d_idxa, d_perm, n_ev, 0, 64, ctx->stream);
  if (e_run == hipSuccess) e_run = rocprim::radix_sort_keys(nullptr, tmp_c, d_begins, d_begins_s, n_chains, 0, 64, ctx->stream);
  if (e_run == hipSuccess) e_run = rocprim::exclusive_scan(nullptr, tmp_scan, d_head, d_rank, (uint64_t)0, n_ev + 1, rocprim::plus<uint64_t>(), ctx->stream);
  HIP_TRY(ctx, e_run);
  void* const d_tmp = cigv_sort_tmp(ctx, std::max(std::max(tmp_a, tmp_b), std::max(tmp_c, tmp_scan))); // (ix.tmp is dead from here)
  if (!d_tmp) return NTS_ENOMEM;
  std::vector<uint64_t> host_first(n_groups + 2); // (the caller's array is written only when the call succeeds)
  if (n_alt) e_run = hipMemcpyAsync(d_alt, alt, n_alt, hipMemcpyHostToDevice, ctx->stream); // (sources of asynchronous copies: a synchronisation follows whatever happens)
  if (e_run == hipSuccess && n_ref) e_run = hipMemcpyAsync(d_ref, ref, n_ref, hipMemcpyHostToDevice, ctx->stream);
  if (e_run == hipSuccess) {
    ScopedTimer t(ctx, "cigar_profile_events", true);
    NTS_LAUNCH(k_cigf_events, IVL_GRID(n_ev), ix.cigar, n_cigar, (const CigPadChain*)d_placed, n_chains, ix.column(0), ix.column(2), ix.column(3),
               ix.column(4), (const uint8_t*)d_alt, n_alt, n_ev, d_key1, d_key2, d_roff);
    e_run = rocprim::radix_sort_pairs(d_tmp, tmp_a, d_key2, d_key2a, iota, d_idxa, n_ev, 0, CIGF_KEY2_BITS, ctx->stream);
    if (e_run == hipSuccess) {
      NTS_LAUNCH(k_cigv_gather, IVL_GRID(n_ev), (const uint64_t*)d_key1, (const uint64_t*)d_idxa, n_ev, d_key1a);
      e_run = rocprim::radix_sort_pairs(d_tmp, tmp_b, d_key1a, d_key1s, d_idxa, d_perm, n_ev, 0, 64, ctx->stream);
    }
    if (e_run == hipSuccess) {
      NTS_LAUNCH(k_cigv_gather, IVL_GRID(n_ev), (const uint64_t*)d_key2, (const uint64_t*)d_perm, n_ev, d_key2s);
      NTS_LAUNCH(k_cigf_chain_keys, IVL_GRID(n_chains), (const CigPadChain*)d_placed, ix.chains, n_chains, d_begins, d_ends);
      e_run = rocprim::radix_sort_keys(d_tmp, tmp_c, d_begins, d_begins_s, n_chains, 0, 64, ctx->stream);
    }
    if (e_run == hipSuccess) e_run = rocprim::radix_sort_keys(d_tmp, tmp_c, d_ends, d_ends_s, n_chains, 0, 64, ctx->stream);
  }
  if (e_run == hipSuccess) {
    ScopedTimer t(ctx, "cigar_profile_emit", true);
    NTS_LAUNCH(k_cigf_heads, IVL_GRID(n_ev + 1), (const uint64_t*)d_key1s, (const uint64_t*)d_key2s, n_ev, d_head);
    e_run = rocprim::exclusive_scan(d_tmp, tmp_scan, d_head, d_rank, (uint64_t)0, n_ev + 1, rocprim::plus<uint64_t>(), ctx->stream);
    if (e_run == hipSuccess)
      NTS_LAUNCH(k_cigd_firsts, IVL_GRID(n_groups + 2), (const uint64_t*)d_key1s, n_ev, (const uint64_t*)d_rank, n_groups, d_col_first);
  }
  if (e_run == hipSuccess) e_run = hipGetLastError();
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(host_first.data(), d_col_first, (n_groups + 2) * 8, hipMemcpyDeviceToHost, ctx->stream);
  e_sync = hipStreamSynchronize(ctx->stream);
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  const uint64_t n_cols = host_first[n_groups];
  if (n_cols == 0 || n_cols > n_ev) return fail(ctx, NTS_EHIP, "nts_cigar_profile: the scan left an impossible number of columns");
  // (the stream is idle: the output's buffer is fetched before its kernel is queued)
  NTS_WS(d_cols, nts_cig_profile_col*, "cigf_cols", n_cols * sizeof(nts_cig_profile_col));
  nts_cig_profile_col* host_cols = (nts_cig_profile_col*)malloc(n_cols * sizeof(nts_cig_profile_col));
  if (!host_cols) return fail(ctx, NTS_ENOMEM, "nts_cigar_profile: no host memory for the columns");
  {
    ScopedTimer t(ctx, "cigar_profile_emit", true);
    NTS_LAUNCH(k_cigf_emit, IVL_GRID(n_ev), (const uint64_t*)d_key1s, (const uint64_t*)d_key2s, (const uint64_t*)d_perm, (const uint64_t*)d_rank,
               (const uint32_t*)d_roff, (const uint8_t*)d_ref, n_ref, (const uint64_t*)d_begins_s, (const uint64_t*)d_ends_s, n_chains,
               (const uint64_t*)d_r0, n_groups, n_ev, d_cols, n_cols);
  }
  e_run = hipGetLastError();
  if (e_run == hipSuccess) e_run = hipMemcpyAsync(host_cols, d_cols, n_cols * sizeof(nts_cig_profile_col), hipMemcpyDeviceToHost, ctx->stream);
  e_sync = hipStreamSynchronize(ctx->stream);
  if (e_run != hipSuccess || e_sync != hipSuccess) free(host_cols);
  HIP_TRY(ctx, e_run);
  HIP_TRY(ctx, e_sync);
  *cols = host_cols;
  memcpy(col_first, host_first.data(), (n_groups + 1) * 8);
  return NTS_OK;
}

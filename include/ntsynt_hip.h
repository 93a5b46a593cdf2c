/*
 * ntsynt_hip.h -- C ABI of libntsynt_hip.so: the MI355X (gfx950) implementation of ntSynt's
 * hot path (canonical-ntHash minimizer sketch + common-k-mer Bloom filter + minimizer-graph
 * chaining).  Plain pointers and sizes only; no exceptions cross this boundary.
 *
 * The reference has no in-process FFI for this path: its boundary is CLI + files
 * (SURVEY.md 8(b)).  Each entry point below names the reference interface it replaces
 * (paths relative to the reference tree); INTEGRATION.md shows the binding a maintainer of the
 * reference would add.
 *
 * Conventions: every call returns 0 on success or a negative code (NTS_E*); the message is
 * retrievable with nts_last_error(ctx) (ctx == NULL: the message of a failed nts_init).
 * Handles are opaque.  One nts_ctx per GPU (owns one HIP stream); a ctx is not thread-safe.
 * Buffers returned through `T**` out-parameters are allocated by the library on the host and
 * released with nts_free().
 */
#ifndef NTSYNT_HIP_H
#define NTSYNT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NTS_OK 0
#define NTS_EINVAL (-22)
#define NTS_ENOMEM (-12)
#define NTS_EHIP (-5)
#define NTS_ERANGE (-34)
#define NTS_EFORMAT (-74) /* input file is not FASTA (e.g. FASTQ) */
#define NTS_ECOMM (-70)   /* RCCL unavailable or a collective failed */

typedef struct nts_ctx nts_ctx;
typedef struct nts_genome nts_genome; /* one FASTA resident in HBM */
typedef struct nts_bf nts_bf;         /* Bloom bit array resident in HBM */
typedef struct nts_mx nts_mx;         /* minimizer list resident in HBM */
typedef struct nts_hset nts_hset;     /* exact set of 64-bit hashes resident in HBM */
typedef struct nts_hcount nts_hcount; /* per member of an nts_hset, how often it was seen: 32-bit counts resident in HBM */
typedef struct nts_comm nts_comm;    /* RCCL communicator of the multi-GPU path (one rank per GPU) */

/* hard-mask interval [start, end) in record coordinates (bedtools maskfasta semantics) */
typedef struct
{
  uint32_t rec;
  uint64_t start;
  uint64_t end;
} nts_interval;

/* ---- context ------------------------------------------------------------------------------- */
int nts_init(int device, nts_ctx** out);
void nts_destroy(nts_ctx* ctx);
const char* nts_last_error(nts_ctx* ctx);
int nts_sync(nts_ctx* ctx);
/* HIP stream of the context (hipStream_t as void*), for callers that enqueue their own work */
void* nts_stream(nts_ctx* ctx);

/* Per-kernel timing with HIP events on the context's stream (bench.py's roofline leg).
 * nts_profile(ctx,1) resets and enables; nts_timing() reports total ms and launch count of the
 * kernel called `name` since then ("hash_probe", "window_min", "bf_insert", ...).  nts_profile(ctx,2) times only
 * the dominant kernels (hash_select, hash_probe, bf_insert): every event pair costs ~10 us of bubble in the stream,
 * which a short call feels.  0 disables. */
int nts_profile(nts_ctx* ctx, int enable);
int nts_timing(nts_ctx* ctx, const char* name, double* total_ms, uint64_t* launches);

/* Device memory of this process's library allocations (all contexts): bytes live now and their high-water mark since the
 * last reset, plus what the device reports as in use / in total (hipMemGetInfo on the context's device: includes other
 * users of the GPU, e.g. a caller's torch tensors).  Replaces the peak-memory column of the reference's `--benchmark`
 * wrappers (`/usr/bin/time -v` / memusg per rule, bin/ntsynt_run_pipeline.smk:26-35; README.md:156-158 quotes wall clock and
 * peak memory per run).  Any out-pointer may be NULL; ctx may be NULL (device figures are then 0).
 * nts_mem_reset_peak: the mark restarts from the bytes live now. */
int nts_mem_stats(nts_ctx* ctx, uint64_t* live_bytes, uint64_t* peak_bytes, uint64_t* device_used_bytes, uint64_t* device_total_bytes);
void nts_mem_reset_peak(void);
/* hipMalloc / hipFree calls the library has made in this process and the host time they took, in ms: what a call that meets a
 * context without workspaces (the first sketch of a run: rule indexlr runs once per genome, bin/ntsynt_run_pipeline.smk:74-85) spends
 * allocating -- bench.py's `cold` leg takes the difference around a call. */
int nts_alloc_stats(uint64_t* calls, double* ms);
/* Device blocks the library frees are kept (up to 96 GB in all) and handed out again, whole or in pieces: on some boxes a hipMalloc of
 * a few hundred MB takes 20-100 ms, memory a process has just given back costs the next allocation a wait, and every genome, filter
 * and context of a run allocates and frees.  Requests below 64 KB live in 8 MB slabs of their own (a long-lived small workspace never
 * holds a large kept allocation).  live / peak of nts_mem_stats count blocks in use, not cached ones (device_used_bytes sees both).
 * nts_mem_trim gives every cached block back to the driver (bytes released); an allocation that fails does so by itself and tries
 * again; so does nts_destroy of the process's last context.  nts_mem_cache_stats: bytes cached now, allocations served from the cache.
 * nts_mem_reserve: ONE driver allocation of `bytes` on `device` (less when the device has less to give; *reserved_bytes says), kept
 * for the allocations to come -- a run that knows its plan (file sizes -> filter, build workspaces, resident genomes) asks the driver
 * once, before its first file is read, and never again; may be called from a thread of its own.  Replaces nothing in the reference
 * (it allocates two filters once, src/ntsynt_make_common_bf.cpp:121-137): it is what makes "allocated once" true of the GPU run.
 * nts_mem_events: out[0..7] = hipMalloc + hipFree calls, ns spent in them, allocations served from the cache, allocations tried again
 * after the cache was emptied, bytes taken from the driver, bytes given back, ns spent waiting for the device before a freed block was
 * kept, nts_mem_reserve calls that got memory (process-wide, monotonic: take differences around a stage). */
uint64_t nts_mem_trim(void);
int nts_mem_cache_stats(uint64_t* cached_bytes, uint64_t* hits);
int nts_mem_reserve(int device, uint64_t bytes, uint64_t* reserved_bytes);
int nts_mem_events(uint64_t out[8]);

/* ---- A1: Bloom filter sizing ----------------------------------------------------------------
 * replaces approximate_bf_size(), src/ntsynt_make_common_bf.cpp:28-40, and the byte rounding of
 * the btllib::KmerBloomFilter constructor used at :122-123.  approx_bytes = ceil(-n/ln(1-fpr))/8
 * (truncating), ctor_bytes = approx_bytes rounded up to a multiple of 8. */
int nts_bf_size_bytes(uint64_t genome_bp, double fpr, uint64_t* approx_bytes, uint64_t* ctor_bytes);
/* The constructor's rounding is recalled from btllib's source, which is not in the reference tree,
 * and it decides the modulus of every bit index: a maintainer holding btllib can settle it by flipping this switch.
 *   NTS_BF_ROUND_UP   ceil(double(bytes) / 8) * 8   -- the default, what nts_bf_size_bytes() returns
 *   NTS_BF_ROUND_DOWN (bytes / 8) * 8               -- an integer division inside the ceil
 *   NTS_BF_ROUND_NONE bytes as approximate_bf_size() returned them
 * Every filter entry point accepts any positive byte count. */
#define NTS_BF_ROUND_UP 0
#define NTS_BF_ROUND_DOWN 1
#define NTS_BF_ROUND_NONE 2
int nts_bf_size_bytes_ex(uint64_t genome_bp, double fpr, int rounding, uint64_t* approx_bytes, uint64_t* ctor_bytes);

/* ---- genome ---------------------------------------------------------------------------------
 * replaces btllib::SeqReader(path, LONG_MODE) record streaming (src/...cpp:32-36,125-131).
 * `seq` = the records' bases concatenated (ASCII, any case, no separators); record r occupies
 * [rec_off[r], rec_off[r]+rec_len[r]).  Copied to HBM once. */
int nts_genome_upload(nts_ctx* ctx,
                      const uint8_t* seq,
                      uint64_t n,
                      const uint64_t* rec_off,
                      const uint64_t* rec_len,
                      uint32_t n_rec,
                      nts_genome** out);
/* A batch of uploaded genomes as one device genome (device-to-device copy): the records of part 0, then those of
 * part 1, ...; record ids of part p start at the number of records of the parts before it.  Sketching the batch is
 * the reference's "indexlr per assembly" (bin/ntsynt_run_pipeline.smk:74-85) for all assemblies with one sequence of launches --
 * records never share k-mers, so the minimizers of a record are those of the same record sketched alone. */
int nts_genome_concat(nts_ctx* ctx, uint32_t n_parts, const nts_genome* const* parts, nts_genome** out);
/* Records [rec0, rec1) of a resident genome as a resident genome of their own (device-to-device copy): the shard one rank of a
 * genome's group works on when genomes < GPUs.  Windows never cross records (Indexlr minimizes per record), so the shards'
 * minimizer lists concatenate to the genome's (nts_mx_concat) and their filters OR to the genome's (nts_bf_allreduce_groups). */
int nts_genome_slice(nts_ctx* ctx, const nts_genome* g, uint32_t rec0, uint32_t rec1, nts_genome** out);
void nts_genome_free(nts_ctx* ctx, nts_genome* g);
/* Bench / scale-test utilities (no counterpart in the reference): a synthetic genome generated directly in
 * HBM -- `n_contigs` equal records of i.i.d. bases drawn from `seed_ancestor`, with independent substitutions
 * at `substitution_rate` keyed by `seed_genome` (genomes sharing seed_ancestor are relatives) -- and the
 * read-back of a slice of any resident genome as upper-case ASCII (concatenated-sequence coordinates). */
int nts_genome_synth(nts_ctx* ctx, uint64_t total_bp, uint32_t n_contigs, uint64_t seed_ancestor, uint64_t seed_genome,
                     double substitution_rate, nts_genome** out);
/* The same family with structural events (inversions, translocations, indels, N runs, so that the block rules
 * of bin/ntsynt_synteny.py:391-409 (indel split), :312-340 (erosion) and :434-472 (collinear merge) have work at full scale):
 * the genome is given as a tiling of pieces in ascending `dst` order -- each a stretch [src, src + len) of the ancestor
 * (coordinates of nts_genome_synth's concatenated ancestor), forwards or reverse-complemented, `len` bases of sequence of the
 * genome's own (an insertion; `src` = offset in that stream), or a run of N -- cut into records of rec_len[r] bases.
 * The plan is the caller's (ntsynt_amd/synth.py structural_plan); substitutions as in nts_genome_synth. */
#define NTS_SYNTH_REVCOMP 1u
#define NTS_SYNTH_NOVEL 2u
#define NTS_SYNTH_NRUN 4u
typedef struct
{
  uint64_t dst, len, src;
  uint32_t flags, reserved;
} nts_synth_piece;
int nts_genome_synth_plan(nts_ctx* ctx, uint32_t n_rec, const uint64_t* rec_len, uint32_t n_pieces, const nts_synth_piece* pieces,
                          uint64_t seed_ancestor, uint64_t seed_genome, double substitution_rate, nts_genome** out);
/* The assembly-like family (BASELINE config 5 stands on real mammalian assemblies, /root/reference README.md:157; they are not in
 * the container): the same tiling, over an ancestor that is not i.i.d.  `rep` describes interspersed repeat families as a function
 * of the ancestor coordinate s -- every cell of 2^cell_log2 bases holds, with probability prob_256/256, one copy of one of
 * `families` consensus elements (SINE-like: sine_len bases; LINE-like: the last line_min_len..line_len bases of a line_len
 * consensus, i.e. 5'-truncated), forwards or reverse-complemented, each copy diverged from its consensus by one of sixteen levels
 * between div_min_1024/1024 and div_max_1024/1024 (young copies share k-mers: within-assembly duplicate minimizers, Bloom buckets
 * that overflow); SINE copies overwrite LINE copies.  Pieces flagged NTS_SYNTH_TANDEM are satellite arrays: `reserved` = the array
 * family, base = that family's sat_unit-base unit at (source coordinate mod sat_unit), diverged at sat_div_1024/1024 per base
 * (keyed by the source coordinate, so that the copies of an array in the genomes of a family agree).  rep == NULL: an i.i.d.
 * ancestor, tandem pieces rejected.  ntsynt_amd/synth.py (realistic_plan, plan_bases) holds the plan and the numpy statement of
 * the same generator that the tests compare with. */
#define NTS_SYNTH_TANDEM 8u
typedef struct
{
  uint32_t sine_cell_log2, sine_len, sine_prob_256, sine_families;
  uint32_t line_cell_log2, line_len, line_min_len, line_prob_256, line_families;
  uint32_t div_min_1024, div_max_1024;
  uint32_t sat_unit, sat_div_1024;
} nts_synth_repeats;
int nts_genome_synth_plan_ex(nts_ctx* ctx, uint32_t n_rec, const uint64_t* rec_len, uint32_t n_pieces, const nts_synth_piece* pieces,
                             uint64_t seed_ancestor, uint64_t seed_genome, double substitution_rate, const nts_synth_repeats* rep,
                             nts_genome** out);
int nts_genome_download(nts_ctx* ctx, const nts_genome* g, uint64_t offset, uint64_t len, uint8_t* ascii);
/* total bases (sum of record lengths, what approximate_bf_size() counts) */
uint64_t nts_genome_bases(const nts_genome* g);
/* number of k-mers made only of A/C/G/T(U), i.e. the k-mers NtHash::roll() visits */
int nts_genome_valid_kmers(nts_ctx* ctx, const nts_genome* g, uint32_t k, uint64_t* n_valid);

/* ---- A2-A4: Bloom filter ----------------------------------------------------------------------
 * nts_bf_create     : btllib::KmerBloomFilter(bytes, 1, k), cpp:122-123,136-137 (bytes = ctor_bytes)
 * nts_bf_insert     : bf->insert(record.seq) over all records, cpp:128-131  (level-1 filter)
 * nts_bf_cascade    : `if (bf->contains(h)) new_bf->insert(h)`, cpp:145-153 (literal cascade level)
 * nts_bf_and        : acc &= other -- with one hash function the cascade equals the AND of the
 *                     per-genome filters; this is the form the multi-GPU path reduces
 * nts_bf_insert_and : one whole cascade level, cpp:134-160, as acc &= (filter of genome g) inside the partitioned build's
 *                     last pass -- no second filter, no clearing, no AND pass; bit for bit what nts_bf_insert into a
 *                     cleared filter followed by nts_bf_and gives (and what nts_bf_cascade gives)
 * nts_bf_popcount   : numerator of bf->get_fpr(), cpp:132,154,162
 * nts_bf_download / nts_bf_upload : raw bit array for bf->save()/load (cpp:164; smk:76).  The download sees
 *                     everything queued before the call and runs on the context's copy stream: it is the one
 *                     call that may be issued from a second host thread while the first keeps sketching. */
int nts_bf_create(nts_ctx* ctx, uint64_t bytes, nts_bf** out);
void nts_bf_free(nts_ctx* ctx, nts_bf* bf);
uint64_t nts_bf_bytes(const nts_bf* bf);
void* nts_bf_device_ptr(nts_bf* bf);
int nts_bf_clear(nts_ctx* ctx, nts_bf* bf);
int nts_bf_insert_and(nts_ctx* ctx, nts_bf* acc, const nts_genome* g, uint32_t k);
int nts_bf_insert(nts_ctx* ctx, nts_bf* bf, const nts_genome* g, uint32_t k);
/* How nts_bf_insert sets the bits (same filter either way): 0 = auto (large genomes: hash, partition the bit
 * indices by filter segment in two streaming passes, set them in LDS bitmaps and OR whole segments into the
 * filter; small ones: one atomic OR per k-mer), 1 = always one atomic OR per k-mer, 2 = partitioned build whenever
 * the filter layout allows it (tests). */
int nts_bf_build_mode(nts_ctx* ctx, int mode);
/* The geometry of the partitioned build for n_valid k-mers of length k and a filter of `bytes` bytes, from the numbers alone (a host
 * function, no GPU: the build itself calls it).  forced: build mode 2; and_mode: the build of nts_bf_insert_and.  Returns 0 when the
 * partitioned build applies and 1 when it does not (no k-mers, 0xFF000000 k-mers or more, a filter beyond 2^37 bits, AND with
 * k > 128, too small to pay for its passes unless forced); out[10] (zeros when it does not apply) = final buckets that hold filter
 * bits F = ceil(bits / 2^19), log2_b2, B2 = 2^log2_b2 <= 512 level-2 buckets per level-1 bucket, B1 = ceil(F / B2) <= 512 level-1
 * buckets, n_final = B1 * B2 final buckets launched (n_final - F < B2 of them lie behind the filter's end), cap1 residues per
 * level-1 bucket, cap2 packed words per level-2 bucket, tiles of the first pass, tiles per level-1 bucket of the second, and
 * idx32 = (B1 * cap1 < 2^32). */
int nts_bf_bin_plan(uint64_t n_valid, uint64_t bytes, uint32_t k, int forced, int and_mode, uint64_t* out);
int nts_bf_cascade(nts_ctx* ctx, const nts_bf* prev, nts_bf* next, const nts_genome* g, uint32_t k);
/* the per-genome loop of the experimental repeat filter (bin/ntsynt_make_repeat_bfs.py:56-67; rule make_repeat_bf,
 * smk:65-72): `if genome_bf.contains(h): repeat_bf.insert(h) else: genome_bf.insert(h)` over every k-mer of g */
int nts_bf_insert_repeats(nts_ctx* ctx, nts_bf* genome_bf, nts_bf* repeat_bf, const nts_genome* g, uint32_t k);
int nts_bf_and(nts_ctx* ctx, nts_bf* acc, const nts_bf* other);
int nts_bf_popcount(nts_ctx* ctx, const nts_bf* bf, uint64_t* bits_set);
int nts_bf_download(nts_ctx* ctx, const nts_bf* bf, uint8_t* host, uint64_t bytes);
int nts_bf_upload(nts_ctx* ctx, nts_bf* bf, const uint8_t* host, uint64_t bytes);
/* bf->save(path) (cpp:164) straight out of HBM: `header` (the caller's btllib-style text header), then the bit array, written
 * by n_threads host threads (0 = default) through pinned staging and positional writes -- no host copy of the filter.
 * Like nts_bf_download it sees everything queued before the call and may run on a second host thread. */
int nts_bf_save(nts_ctx* ctx, const nts_bf* bf, const char* path, const void* header, uint64_t header_bytes, uint32_t n_threads);
/* Microbenchmark: n_probes pseudo-random single-bit reads of the filter with the access shape of the sketch's
 * probe batches and no hashing -- the empirical ceiling for sector-granular random reads on this GPU. */
int nts_bench_random_probe(nts_ctx* ctx, const nts_bf* bf, uint64_t n_probes, uint32_t repeats, double* avg_ms, uint64_t* hits);
/* Microbenchmark: issue rate of the integer VALU instructions ntHash is made of (the roof of the VALU-bound kernels
 * k_hash_select and k_bin1).  kind: 0 v_xor_b32, 1 v_alignbit_b32, 2 v_lshl_add_u64, 3 v_lshlrev_b64, 4 v_mul_lo_u32,
 * 5 v_mad_u64_u32, 6 v_add_co_u32 + v_addc_co_u32 (a 64-bit add as two instructions), 7 a dependent chain of v_xor_b32
 * (latency).  Every CU runs `waves_per_simd` (1..8) waves per SIMD, each wave `instr_per_wave` instructions in eight
 * independent chains; cycles_per_instr = shader cycles (s_memtime) a SIMD needs per wave-instruction; wall_ms = the
 * launch, from which wave-instructions per second per CU = 4 * waves_per_simd * instr_per_wave / wall follow. */
int nts_bench_valu(nts_ctx* ctx, int kind, uint32_t waves_per_simd, uint32_t iters, double* wall_ms, double* cycles_per_instr,
                   double* instr_per_wave);
/* Diagnostic: out[i] = h[i] mod bits computed by the device code every probe and insert goes through (nts::FastMod: a
 * generic form and two short ones for bits > 2^32 and 2^32 < bits < 2^38; `form` = -1 takes the one the library would, 0..2
 * caps it) -- btllib's `hashes[0] % array_bits`.  h and out are host arrays of n words. */
int nts_mod_indices(nts_ctx* ctx, uint64_t bits, int form, const uint64_t* h, uint64_t n, uint64_t* out);
/* Non-owning filter over caller-provided HBM (e.g. the buffer a collective runs on): `device_ptr` must be
 * 16-byte aligned and hold `bytes` rounded up to a multiple of 16, the tail zeroed.  nts_bf_free() on a
 * wrapped filter releases only the handle. */
int nts_bf_wrap(nts_ctx* ctx, void* device_ptr, uint64_t bytes, nts_bf** out);
/* acc &= other on raw device buffers (bytes a multiple of 16): the local reduction step of the
 * bitwise-AND all-reduce of per-genome filters across GPUs (SURVEY.md 8(e) exchange 1; RCCL has no
 * bitwise reduction). */
int nts_and_raw(nts_ctx* ctx, void* acc_dev, const void* other_dev, uint64_t bytes);

/* ---- multi-GPU exchange steps: one process per GPU, genomes partitioned over the ranks -------------
 * The reference has no counterpart (it is a single-node Snakemake workflow); these calls are what a sharded
 * make_common_bf (src/ntsynt_make_common_bf.cpp:134-160) and the hand-over of the per-genome indexlr outputs to
 * ntsynt_run.py (bin/ntsynt_run_pipeline.smk:87-103) become across GPUs.
 *
 * nts_comm_unique_id : 128 opaque bytes (ncclGetUniqueId) made on one rank and handed to all by the launcher
 *                      (torch.distributed store, MPI, a file)
 * nts_comm_init      : ncclCommInitRank on the context's GPU
 * nts_comm_wrap      : adopt an existing ncclComm_t (not destroyed by nts_comm_destroy)
 * nts_comm_library   : which library serves the collectives: "librccl" (the process's copy or the system's), the path
 *                      given in NTS_RCCL_LIB (a site's own build; the test suite's stand-in for ranks that share one
 *                      GPU), or "" when none could be loaded.  (The environment variables the product build reads are four:
 *                      NTS_RCCL_LIB, NTS_COMM_PIECE, NTS_IO_THREADS, NTS_HOST_THREADS -- csrc/nts_knobs.h; NTS_COMM_PIECE and
 *                      NTS_IO_THREADS are read ONCE per context, by nts_init: set them before the context is created.  The
 *                      experiment switches exist only in libntsynt_hip_exp.so.)
 * nts_bf_create_sharded : a filter whose allocation is `world` chunks of a multiple of 16 bytes -- the layout the
 *                      all-reduce exchanges; otherwise identical to nts_bf_create
 * nts_bf_fill_ones   : identity of AND, for a rank that owns no genome
 * nts_bf_allreduce_and : exchange 1 -- in place, every rank ends with the bitwise AND of all ranks' filters (= the
 *                      cascade's result).  RCCL has no bitwise reduction: direct reduce-scatter with
 *                      ncclSend/ncclRecv over all xGMI links at once through a (world-1) x 256 MiB scratch, a local AND
 *                      kernel, ncclAllGather in place.  comm == NULL or world 1: no-op.
 * nts_mx_allgather   : exchange 2 -- the ranks' minimizer lists (n_local handles, genome numbers in local_ids; a rank
 *                      holds at most ceil(n_total / world)) gathered on every rank: out[g] = list of genome g,
 *                      resident in HBM, g in [0, n_total); released with nts_mx_free.  Two collectives per call. */
int nts_comm_unique_id(uint8_t* id128);
int nts_comm_init(nts_ctx* ctx, const uint8_t* id128, int world, int rank, nts_comm** out);
int nts_comm_wrap(nts_ctx* ctx, void* rccl_comm, nts_comm** out);
void nts_comm_destroy(nts_comm* comm);
int nts_comm_world(const nts_comm* comm);
int nts_comm_rank(const nts_comm* comm);
void* nts_comm_handle(const nts_comm* comm);
const char* nts_comm_library(void);
int nts_bf_create_sharded(nts_ctx* ctx, uint64_t bytes, int world, nts_bf** out);
int nts_bf_fill_ones(nts_ctx* ctx, nts_bf* bf);
int nts_bf_allreduce_and(nts_ctx* ctx, nts_bf* bf, nts_comm* comm);
/* Exchange 1 when there are fewer genomes than GPUs (last paragraph; what the reference parallelises over is
 * records, src/ntsynt_make_common_bf.cpp:128-131,145-153): the ranks of group g hold the filters of the shards (record ranges,
 * nts_genome_slice) of genome g.  In place, every rank ends with AND over groups of (OR over the group's ranks); group_of[r] in
 * [0, n_groups) for each of the communicator's ranks, every group with at least one rank.  group_of == NULL: nts_bf_allreduce_and.
 * nts_comm_last_sparse: 1 if the context's last all-reduce gathered the set bits' indices instead of the reduced chunks (a
 * reduced filter that is all but empty -- BASELINE config 4 -- moves megabytes instead of the filter's size). */
int nts_bf_allreduce_groups(nts_ctx* ctx, nts_bf* bf, nts_comm* comm, const int32_t* group_of, uint32_t n_groups);
int nts_comm_last_sparse(const nts_ctx* ctx);
/* The context's last exchange 2 (nts_mx_allgather[_ex]): the lists travel packed -- h1 as it is, the position in 32 bits when the
 * list's largest fits, the record as one start index per RECORD (a list is in record order): 12 bytes per minimizer and a few KB where
 * the lists themselves hold 20.  packed_bytes / unpacked_bytes: all ranks' lists in the two forms; sent_bytes: what this rank sent. */
int nts_comm_last_exchange2(const nts_ctx* ctx, uint64_t* packed_bytes, uint64_t* unpacked_bytes, uint64_t* sent_bytes);
/* Exchange 1 when a family's records are shared out over the ranks by bases, across genome boundaries (ntsynt_amd/pipeline.py
 * partition_plan: three genomes on eight GPUs are eight ranges of 1.125 Gbp, not 3/3/2 ranks per genome): a rank holds one filter per
 * genome its range of records touches.  bfs[0 .. n_local): this rank's filters, all of one size (nts_bf_create_sharded); the first
 * n_of[rank] of them are contributions, and bfs[0] receives the result on every rank (a rank without records still passes one
 * filter, the destination).  slot_group[r * n_slots + s] = group (genome) of rank r's s-th filter, -1 = none (a rank's contributions
 * are its first slots); every group in [0, n_groups) needs a filter somewhere; at most 128 filters in all.  Result as
 * nts_bf_allreduce_groups: AND over groups of (OR over the group's filters) -- the reference's cascade with the OR of
 * src/ntsynt_make_common_bf.cpp:128-131 (the records of a file inserted into one filter) spread over ranks.  comm == NULL or world 1:
 * the reduction over this rank's own filters. */
int nts_bf_allreduce_parts(nts_ctx* ctx, nts_bf* const* bfs, uint32_t n_local, nts_comm* comm, uint32_t n_slots, const int32_t* slot_group,
                           uint32_t n_groups);
int nts_mx_allgather(nts_ctx* ctx, nts_comm* comm, uint32_t n_local, const nts_mx* const* local, const uint32_t* local_ids,
                     uint32_t n_total, nts_mx** out);
/* nts_mx_allgather with the list slots per rank said by the caller (0: ceil(n_total / world)): with records shared out by bases a
 * rank holds one list per genome its range touches, and the plan's maximum is the slot count on every rank. */
int nts_mx_allgather_ex(nts_ctx* ctx, nts_comm* comm, uint32_t n_local, const nts_mx* const* local, const uint32_t* local_ids,
                        uint32_t n_total, uint32_t slots_per_rank, nts_mx** out);

/* ---- B1-B3, B5: minimizer sketch -----------------------------------------------------------------
 * replaces `indexlr -k K -w W --long --pos -s common.bf genome.fa` (smk:81-85) and the re-sketch of
 * hard-masked assemblies in the refinement rounds (bin/ntsynt_synteny.py:134-157,167-192): the mask
 * intervals are applied to the resident sequence instead of writing masked FASTA files.
 * Result: minimizers in (record, position) order; h1 = the hash indexlr prints. */
int nts_sketch(nts_ctx* ctx,
               const nts_genome* g,
               uint32_t k,
               uint32_t w,
               const nts_bf* filter_or_null,
               const nts_interval* mask,
               uint64_t n_mask,
               nts_mx** out);

/* The same with a filter-out Bloom filter as well (`indexlr -r <bf>`, the reference's experimental repeat filter: rule indexlr,
   bin/ntsynt_run_pipeline.smk:74-85, and ntsynt_synteny.py:172-180): a k-mer present in `filter_out` is rejected like one
   absent from `filter`; either may be NULL.  With a filter-out filter the call takes the every-k-mer-probed kernels. */
int nts_sketch_ex(nts_ctx* ctx, const nts_genome* g, uint32_t k, uint32_t w, const nts_bf* filter, const nts_bf* filter_out,
                  const nts_interval* mask, uint64_t n_mask, nts_mx** out);
/* Sketch policy.  mode 0 = auto (pruned when w >= 200 and c = 11 / accepted share stays below w/4, below 0.15 w for w < 512; for
 * 8 <= w < 200 the tiered selection, nts_sketch_tiers, where its estimated probes pay -- always so without a filter),
 * 1 = dense (probe the filter for every k-mer), 2 = pruned: only k-mers whose hash is <= (c / w) * 2^64 are probed;
 * windows holding no accepted candidate are re-evaluated densely, so the result is identical
 * (ntsynt_amd/csrc/nts_pruned.inc).  prune_c = 0: c is chosen per call from the filter's occupancy
 * (c = 11 / accepted share, at least 8: DESIGN.md 4.1); otherwise c = prune_c. */
int nts_sketch_mode(nts_ctx* ctx, int mode, uint32_t prune_c);
/* Dense sketch over a sparse filter (many divergent genomes: nearly no k-mer is common to all): when occupancy x 2^shift is
 * small, a summary of the filter with one bit per 2^shift filter bits (<= 4 MiB: mostly L2-resident; built once per filter state) is
 * consulted first and only a set summary bit leads to a read of the filter; key tiles without an accepted k-mer are skipped
 * by the window kernel.  In auto mode the accepted k-mers themselves become the candidate list (no keys, no window kernel), and
 * when the filter holds few enough set bits a copy of it folded onto 2^19 bits is looked at first, from LDS.  Identical output.
 * mode 0 = auto (default), 1 = never, 2 = auto without the LDS copy, -1 = leave as is; last_shift = the shift the last
 * nts_sketch call used (0: it did not use a summary). */
int nts_sketch_summary(nts_ctx* ctx, int mode, uint32_t* last_shift);
/* Candidate selection of the pruned sketch (k_hash_select_hi / k_hash_select): 0 = automatic (the kernel that rolls only the
   upper halves of the strand hashes where it applies -- k <= 32, at most ~180 candidates per 4096 k-mers -- and pays -- fewer
   than one run of valid bases per two tiles), 1 = always the full-width kernel, 2 = the upper-halves kernel wherever it
   applies, fragmented assemblies included.  Results are identical; tests and measurements switch it. */
int nts_sketch_select(nts_ctx* ctx, int impl);
/* Tiered selection (k_hash_tiers, ntsynt_amd/csrc/nts_tiers.inc): for filters that accept a few per cent of a genome's k-mers
 * (three genomes at 10 % divergence, eight at 4 %, the reference's eleven-genome benchmark row, README.md:158) one threshold would list a
 * quarter of the k-mers or more.  Thresholds tau_0 2^t, t = 0, 1, ..., are then probed one after the other, each only where
 * some window still holds no accepted k-mer: ~3.4 / p probes per window instead of 11 / p (p = accepted share), identical
 * output (the filter-in semantics of indexlr -s, bin/ntsynt_run_pipeline.smk:81-85).  mode 0 = automatic (default), 1 = never,
 * 2 = wherever the kernel applies, -1 = leave as is; x0 = accepted k-mers per window the first tier aims at (0: default 2.4, 1.2 for
 * w < 64).  Automatic also means: short windows (8 <= w < 64, the last refinement round's w = 10, bin/ntSynt:89-91) go this way while the
 * filter accepts about five k-mers per window -- a fifth to a half of the probes of the every-k-mer pass;
 * half_steps: thresholds grow by 1.5 / 1.33 instead of 2.  Of the last nts_sketch call that went this way: k-mers probed,
 * rounds run summed over the tiles, tiers planned (0: it did not go this way). */
int nts_sketch_tiers(nts_ctx* ctx, int mode, double x0, int half_steps, uint64_t* last_probes, uint64_t* last_rounds, uint32_t* last_tiers);
/* of the last nts_sketch call: accepted candidates, uncovered ranges handed to the dense kernels, the number of
 * k-mers in them, and the c that was used (all 0 for a dense-mode call) */
int nts_sketch_stats(nts_ctx* ctx, uint64_t* candidates, uint64_t* uncovered_ranges, uint64_t* uncovered_kmers, uint32_t* prune_c_used);
/* Which of the paths for repeat-rich or fragmented input the last calls took (tests assert that an assembly-like family reaches
 * them): of the last nts_sketch call, the candidates of k_hash_select_hi tiles that listed more k-mers than their slots hold (the
 * two-sweep path: copies of a repeat, tiles in pieces); of the last partitioned Bloom build (nts_bf_insert / nts_bf_insert_and), the
 * indices that bypassed the buckets (a full bucket: the copies of a repeat family; lanes whose k-mers span a run boundary), and
 * whether its list of such indices ran full (store-only build: fell back to read-and-OR on the device; fused AND build: redone
 * with a filter of the genome's own).  The Bloom figures are read at the next synchronising call on the filter
 * (nts_bf_popcount, nts_bf_download, nts_sync). */
int nts_path_stats(nts_ctx* ctx, uint64_t* sketch_many_listed, uint64_t* bf_direct_indices, uint32_t* bf_list_fallback);
/* Of the last partitioned Bloom build on this context (tests assert the shape a case was built for): the workgroups its first pass
 * k_bin1 was launched with (min(tiles, 2 per CU); 0 when the build did not apply or k > 128 took the run-table walk), its level-1
 * buckets B1 and log2 of its level-2 buckets per level-1 bucket (nts_bf_bin_plan). */
int nts_bf_bin_last(nts_ctx* ctx, uint32_t* bin1_workgroups, uint32_t* B1, uint32_t* log2_b2);
/* The same with one figure more: the idx32 the launch was given (1: a residue's place in the level-1 array is a 32-bit index, what the
 * plan says for B1 * cap1 < 2^32; 0: the general 64-bit place -- beyond ~3.8 G k-mers, or NTS_BIN_IDX32=0 on the experiments build). */
int nts_bf_bin_last_ex(nts_ctx* ctx, uint32_t* bin1_workgroups, uint32_t* B1, uint32_t* log2_b2, uint32_t* idx32);
/* Of the last nts_bf_insert_and: whether the level went the literal way of src/ntsynt_make_common_bf.cpp:134-160 -- every k-mer of
 * the genome looked up in the running filter, the bits that were hit kept -- which the library chooses by itself once the running
 * filter is all but empty (its popcount known and below ~6 * 10^5 bits, where two folded tables in LDS answer most look-ups: what is
 * left of BASELINE configs[3]'s filter after its eighth genome), and how many k-mers were accepted.  Otherwise the level is the partitioned build with the AND in its last pass.
 * Same bits either way (tests/test_gpu_parity.py).  NTS_BF_SPARSE_LEVEL=0 in the environment keeps every level on the build. */
int nts_bf_level_stats(nts_ctx* ctx, uint32_t* sparse_level, uint64_t* accepted_kmers);
uint64_t nts_mx_count(const nts_mx* mx);
void nts_mx_free(nts_ctx* ctx, nts_mx* mx);
/* copy a minimizer list to caller-provided host arrays of nts_mx_count() elements */
int nts_mx_download(nts_ctx* ctx, const nts_mx* mx, uint64_t* h1, uint32_t* rec, uint64_t* pos);
/* device pointers (for an all-gather over RCCL): arrays of nts_mx_count() elements */
int nts_mx_device_ptrs(const nts_mx* mx, void** h1, void** rec, void** pos);
/* device-to-device copy into caller buffers of nts_mx_count() elements (send side of the all-gather) */
int nts_mx_export(nts_ctx* ctx, const nts_mx* mx, void* h1_dev, void* rec_dev, void* pos_dev);
/* the same without waiting: the copies are queued on the context's stream; nts_sync() before the buffers are read
 * by another stream and before the list is freed (several lists, one wait) */
int nts_mx_export_async(nts_ctx* ctx, const nts_mx* mx, void* h1_dev, void* rec_dev, void* pos_dev);
/* k-mer text (upper case, k bytes per minimizer, no separators) of a list sketched from `g`, to a host buffer of
 * nts_mx_count() * k bytes: what `indexlr --seq` prints (smk:81) when the host never held the bases (nts_genome_from_fasta) */
int nts_mx_kmers(nts_ctx* ctx, const nts_genome* g, const nts_mx* mx, uint32_t k, uint8_t* host);
/* the list of a batch genome (nts_genome_concat) taken apart on the device: out[p] = the minimizers of records
 * [rec_base[p], rec_base[p+1]) with record ids rebased to the part (rec_base has n_parts + 1 entries) */
int nts_mx_split(nts_ctx* ctx, const nts_mx* mx, uint32_t n_parts, const uint32_t* rec_base, nts_mx** out);
/* the inverse: the lists of a genome's shards (nts_genome_slice), in record order, as the genome's list -- part p's record
 * numbers raised by rec_offset[p] */
int nts_mx_concat(nts_ctx* ctx, uint32_t n_parts, const nts_mx* const* parts, const uint32_t* rec_offset, nts_mx** out);
/* ntJoin's read_minimizers(file, repeat_bf) -- stage 3's `--filter Filter --repeat <bf>` (bin/ntsynt_synteny.py:183-184,601-604; the
 * function itself is ntJoin's and not in the reference tree: [RECALLED]): *out = the minimizers of `mx` whose k-mer
 * (k bases of `g` at the minimizer's record and position) the filter does NOT hold, in order; released with nts_mx_free. */
int nts_mx_screen(nts_ctx* ctx, const nts_genome* g, const nts_mx* mx, uint32_t k, const nts_bf* filter_out, nts_mx** out);
/* build a device list from host arrays (receiving side of the all-gather, tests) */
int nts_mx_upload(nts_ctx* ctx,
                  const uint64_t* h1,
                  const uint32_t* rec,
                  const uint64_t* pos,
                  uint64_t n,
                  nts_mx** out);

/* test/bench hook: canonical h0 of every valid k-mer in (record, position) order (row B1) */
int nts_hash_all(nts_ctx* ctx, const nts_genome* g, uint32_t k, uint64_t** h0, uint64_t* n_out);

/* The s smallest DISTINCT canonical ntHash values (h0, as nts_hash_all returns them) over the valid k-mers of g,
 * ascending; *n_out = min(s, number of distinct values).  h0 == UINT64_MAX is never part of a sketch (sentinel).
 * Exact (a bottom-s MinHash sketch, the input of the Mash distance in ntsynt_amd/divergence.py); `out` holds s values. */
int nts_minhash(nts_ctx* ctx, const nts_genome* g, uint32_t k, uint32_t s, uint64_t* out, uint32_t* n_out);

/* ---- assessment of synteny blocks ---------------------------------------------------------------------
 * The block statistics of the reference's analysis_scripts/denovo_synteny_block_stats.py (README "Basic assessment of synteny
 * blocks") are host arithmetic over the block table and the .fai files: ntsynt_amd/assess.py block_stats, bin/ntsynt_block_stats.
 * The two calls below have no counterpart there: they give the Mash distance of `-d auto` (nts_minhash) per block.
 *
 * nts_minhash_intervals: the bottom-s sketch of each of n_iv intervals of g in one sweep.  For interval i, out[i * s ..] holds the
 *   n_out[i] = min(s, distinct) smallest DISTINCT canonical h0, ascending, over the valid k-mers that lie wholly inside
 *   [start, end) of record rec (start <= p and p + k <= end; end is clipped to the record length); n_kmers[i] (may be NULL) = how
 *   many such k-mers there are.  Hashing as nts_minhash / nts_hash_all; exact.  Intervals in any order, overlapping, shorter than
 *   k (an empty sketch).  NTS_EINVAL for a record index out of range.  Any k >= 1; s >= 1.  Memory: at most 256 s bytes of hash
 *   sets per interval, the intervals taken in chunks of 2 GiB of them (csrc/nts_minhash_iv.inc).
 * nts_minhash_intervals_stats: of the last call on ctx -- the sweeps of the chunk that took most (1: every threshold held at once),
 *   the chunks, the sweeps of all chunks (each sweep is one launch of the timer "minhash_iv").
 * nts_minhash_pairs: sk = n_sketches sketches of s slots each (n_sk[i] <= s of them used, ascending, distinct: as the call above
 *   returns them), all in host memory.  For pair p of sketches A = pair_a[p], B = pair_b[p]: usize[p] = |bottom-s(A u B)|,
 *   shared[p] = |bottom-s(A u B) n A n B| -- the two integers of the Mash distance (ntsynt_amd/divergence.py). */
int nts_minhash_intervals(nts_ctx* ctx, const nts_genome* g, uint32_t k, uint32_t s, const nts_interval* iv, uint64_t n_iv, uint64_t* out,
                          uint32_t* n_out, uint64_t* n_kmers);
int nts_minhash_intervals_stats(nts_ctx* ctx, uint32_t* passes, uint32_t* chunks, uint64_t* sweeps);
int nts_minhash_pairs(nts_ctx* ctx, uint32_t s, const uint64_t* sk, const uint32_t* n_sk, uint64_t n_sketches, const uint64_t* pair_a,
                      const uint64_t* pair_b, uint64_t n_pairs, uint32_t* shared, uint32_t* usize);

/* ---- what the blocks leave out: gap content ----------------------------------------------------------
 * nts_bf_count_intervals: for interval i of g, n_kmers[i] = the valid k-mers that lie wholly inside [start, end) of record rec
 *   (the rule, the clipping and the NTS_EINVAL of nts_minhash_intervals) and n_hits[i] = how many of them bf holds: bit
 *   h0 mod (8 * bytes) of the filter, h0 the canonical hash as nts_bf_insert and the sketch form it (one hash function).  Exact, every
 *   k-mer probed once, one sweep for all intervals of the call (timer "bf_count_iv", one launch per 2^23 tiles of 8192 k-mers).
 *   Intervals in any order, overlapping, shorter than k (both counts 0).  Any k >= 1.  ntsynt_amd/gaps.py, `ntSynt --gaps`,
 *   bin/ntsynt_gaps; csrc/nts_bf_iv.inc.
 * nts_genome_valid_bases: n_valid[i] = the A/C/G/T bases of interval i (the rest of its length is N or another letter), from the
 *   genome's table of valid stretches on the host: no GPU work. */
int nts_bf_count_intervals(nts_ctx* ctx, const nts_genome* g, uint32_t k, const nts_bf* bf, const nts_interval* iv, uint64_t n_iv,
                           uint64_t* n_kmers, uint64_t* n_hits);
int nts_genome_valid_bases(nts_ctx* ctx, const nts_genome* g, const nts_interval* iv, uint64_t n_iv, uint64_t* n_valid);

/* ---- where a gap's shared sequence lies in the other genomes: gap links -------------------------------
 * nts_bf_sample_intervals: the sibling of nts_bf_count_intervals that writes survivors instead of counting them.  A k-mer of
 *   interval i is sampled when it is valid and lies wholly inside the interval (the counting call's rule, clipping and NTS_EINVAL),
 *   bf holds it (bit h0 mod (8 * bytes)) and h0 <= UINT64_MAX / rate (integer division; rate >= 1, rate 1 samples every k-mer the
 *   filter holds).  n_sampled[i] = how many there are; *out = their records in interval order, then k-mer order -- iv = i, off = the
 *   k-mer's position minus the interval's start (the start clipped to the record) --, *n_out of them; (NULL, 0) when there is none.
 *   Released with nts_free().  Two launches per 2^23 tiles (timers "bf_sample_count", "bf_sample_write"), no atomic: the output is
 *   deterministic.  NTS_ERANGE for an interval of 2^32 bases or more and for 2^32 records or more.  csrc/nts_bf_sample.inc.
 * nts_iv_links: n_lists (at most 64) arrays of such records, one per genome (iv = the interval's index within that genome's
 *   list), joined by hash.  A hash is usable when no list has it more than once; an anchor of interval a (list A) and interval b
 *   (list B, A < B) is a usable hash in both; a link is a pair (a, b) with at least min_anchors (>= 1) anchors.  Per link: anchors;
 *   the smallest and largest off of its anchors in a and in b; fwd / rev = with the anchors ordered by off in a (equal offsets,
 *   which one sweep's records never have within a link, by hash), the consecutive pairs whose off in b rises / falls.  *out = the
 *   links sorted by (list_a, iv_a, list_b, iv_b), *n_out of them; (NULL, 0) for no link, an empty input or a single list.  Released
 *   with nts_free().  Radix sorts, scans and a reduction by key on the context's stream (timers "iv_links_join", "iv_links_pairs",
 *   "iv_links_select"); NTS_ERANGE for 2^32 records, intervals or anchor pairs or more.  csrc/nts_iv_links.inc.
 *   ntsynt_amd/gaps.py links, `ntSynt --gap-links`, `bin/ntsynt_gaps --links-out`. */
typedef struct
{
  uint64_t h0;
  uint32_t iv;
  uint32_t off;
} nts_sample;
typedef struct
{
  uint32_t list_a, iv_a, list_b, iv_b;
  uint32_t anchors, fwd, rev;
  uint32_t min_off_a, max_off_a, min_off_b, max_off_b;
} nts_iv_link;
int nts_bf_sample_intervals(nts_ctx* ctx, const nts_genome* g, uint32_t k, const nts_bf* bf, uint64_t rate, const nts_interval* iv,
                            uint64_t n_iv, uint64_t* n_sampled, nts_sample** out, uint64_t* n_out);
int nts_iv_links(nts_ctx* ctx, uint32_t n_lists, const nts_sample* const* lists, const uint64_t* n, uint32_t min_anchors, nts_iv_link** out,
                 uint64_t* n_out);

/* ---- where a gap's shared sequence lies inside the blocks: gap block links ---------------------------
 * nts_hset_build: an exact set of the n 64-bit values of the host array h (duplicates allowed; n = 0: the empty set), in device memory
 *   from the context's allocator: open addressing, at most half full, 8 bytes per slot; the home slot mixes every bit of the value
 *   (values under a sampling threshold have their top bits zero).  Built by one kernel with 64-bit compare-and-swap: the order of
 *   the slots may differ from run to run, membership does not.  Exact for every value, 0 and 2^64 - 1 included.  Timer
 *   "hset_build".  NTS_ERANGE for more than 2^31 values.  Released with nts_hset_free().
 * nts_hset_contains: out[i] = 1 when h[i] is a member, 0 otherwise (host arrays; fewer than 2^32 queries per call).
 * nts_hset_sample_intervals: nts_bf_sample_intervals with "the set has h0" in place of "the filter holds h0": the same records in
 *   the same order, the same clipping, NTS_EINVAL and NTS_ERANGE, two launches per 2^23 tiles (timers "hset_sample_count",
 *   "hset_sample_write"), no atomic, deterministic; *out released with nts_free().  The threshold is tested first: one k-mer in
 *   `rate` touches the table.  csrc/nts_hset.inc; ntsynt_amd/gaps.py block_links, `ntSynt --gap-block-links`,
 *   `bin/ntsynt_gaps --block-links-out`. */
int nts_hset_build(nts_ctx* ctx, const uint64_t* h, uint64_t n, nts_hset** out);
void nts_hset_free(nts_ctx* ctx, nts_hset* set);
int nts_hset_contains(nts_ctx* ctx, const nts_hset* set, const uint64_t* h, uint64_t n, uint8_t* out);
int nts_hset_sample_intervals(nts_ctx* ctx, const nts_genome* g, uint32_t k, const nts_hset* set, uint64_t rate, const nts_interval* iv,
                              uint64_t n_iv, uint64_t* n_sampled, nts_sample** out, uint64_t* n_out);

/* ---- how often each genome holds a gap's sampled k-mers: gap copies ----------------------------------
 * nts_hcount_create: a counter for `set`: one uint32 per slot of the set's table and one for the value 2^64 - 1, in device memory
 *   from the context's allocator, all zero.  It belongs to that set: every other call takes both, and NTS_EINVAL when they do not
 *   match.  Free the counter before its set.  Released with nts_hcount_free() (NULL: nothing happens).
 * nts_hcount_clear: every count back to zero, and the running total (below) with them.  Timer "hcount_clear".
 * nts_hcount_add: every h[i] (host array) that is a member of the set adds 1 to its count; a non-member adds nothing.  One lane per
 *   value, the set's own walk, one 32-bit atomic add on global memory per member.  Timer "hcount_add".
 * nts_hset_count_intervals: for every valid k-mer that lies wholly inside interval i of g (the rule, the clipping and the NTS_EINVAL
 *   of nts_hset_sample_intervals) with h0 <= UINT64_MAX / rate and h0 in the set: 1 to that member's count and 1 to n_hits[i].
 *   Overlapping intervals count a k-mer once per interval; counts accumulate over calls until cleared.  One launch per 2^23 tiles
 *   (timer "hcount_sweep"): the sampling sweep's probe, then one atomic add per hit, its result unused; n_hits through one plain
 *   store per tile.  Integer adds commute: counts are exact and the same from run to run.
 * nts_hcount_read: out[i] = the count of h[i], 0 for a non-member (host arrays; fewer than 2^32 queries per call).  The order of the
 *   set's slots differs from run to run, so counts are only ever read by key.
 * Range: counts are 32-bit.  The counter keeps on the host how many values (nts_hcount_add: n) and k-mers (nts_hset_count_intervals:
 *   every k-mer of the intervals, hit or not) it has been offered since the last clear; a call that would bring that total to 2^32 or
 *   more is refused with NTS_ERANGE before anything is launched (and before h is read).
 *   csrc/nts_hcount.inc; ntsynt_amd/gaps.py copies, `ntSynt --gap-copies`, `bin/ntsynt_gaps --copies-out`. */
int nts_hcount_create(nts_ctx* ctx, const nts_hset* set, nts_hcount** out);
int nts_hcount_clear(nts_ctx* ctx, nts_hcount* cnt);
void nts_hcount_free(nts_ctx* ctx, nts_hcount* cnt);
int nts_hcount_add(nts_ctx* ctx, const nts_hset* set, nts_hcount* cnt, const uint64_t* h, uint64_t n);
int nts_hcount_read(nts_ctx* ctx, const nts_hset* set, const nts_hcount* cnt, const uint64_t* h, uint64_t n, uint32_t* out);
int nts_hset_count_intervals(nts_ctx* ctx, const nts_genome* g, uint32_t k, const nts_hset* set, nts_hcount* cnt, uint64_t rate,
                             const nts_interval* iv, uint64_t n_iv, uint64_t* n_hits);

/* ---- where each genome holds the copies of a gap: gap copy sites --------------------------------------
 * nts_hset_sample_intervals_capped: nts_hset_sample_intervals with "the set has h0 and 1 <= its count in cnt <= cap" in place of "the
 *   set has h0": the same records in the same order (interval order, then k-mer order), the same clipping, NTS_EINVAL and
 *   NTS_ERANGE, two launches per 2^23 tiles (timers "hcount_sample_count", "hcount_sample_write"), no atomic, deterministic; *out
 *   released with nts_free().  cnt is the set's own counter (NTS_EINVAL otherwise, and for cap = 0 or rate = 0) and is only read:
 *   its counts and its running total stay what they are.  Per member under the threshold, one dependent 4-byte load of the count
 *   behind the set's walk.  With cap = 2^32 - 1 after a count sweep of the same intervals the records are those of
 *   nts_hset_sample_intervals.  csrc/nts_hcount.inc.
 * nts_iv_sites: n_lists (at most 64) arrays of query records as for nts_iv_links (iv = the gap's index within its list), joined by
 *   hash against ONE target genome's occurrence records (iv = record index, off = position in the record), multiplicity allowed on
 *   both sides: a pair is a query record q and a target record o of one hash (a hash a gap has twice and the target three times
 *   gives six pairs).  For one gap, its pairs ordered by (o.iv, o.off, q's place in its list), a site is a maximal run of
 *   consecutive pairs with equal o.iv whose consecutive o.off differ by at most `step`.  Per site: hits = its pairs; first_t /
 *   last_t = the smallest / largest o.off; min_off_q / max_off_q = the smallest / largest q.off; fwd / rev = the consecutive pairs of
 *   the site, in that order, whose q.off rises / falls (equal: neither).  *out = the sites with hits >= min_hits (>= 1) sorted by
 *   (list_q, iv_q, rec_t, first_t), *n_out of them; (NULL, 0) for no site, an empty target, an empty list or no list.  Released with
 *   nts_free().  One radix sort of the target, a lower / upper bound per query record, a scan, ONE LANE PER PAIR to write the
 *   pairs, two stable radix sorts, a scan and a reduction by key, all on the context's stream and in its workspace, no atomic and
 *   no launch per gap (timers "iv_sites_join", "iv_sites_pairs", "iv_sites_select"); NTS_ERANGE for 2^32 records, gaps or pairs
 *   or more.  csrc/nts_iv_sites.inc; ntsynt_amd/gaps.py copy_sites, `ntSynt --gap-copy-sites`, `bin/ntsynt_gaps --copy-sites-out`. */
typedef struct
{
  uint32_t list_q, iv_q, rec_t;
  uint32_t hits, fwd, rev;
  uint32_t min_off_q, max_off_q, first_t, last_t;
} nts_iv_site;
int nts_hset_sample_intervals_capped(nts_ctx* ctx, const nts_genome* g, uint32_t k, const nts_hset* set, const nts_hcount* cnt, uint32_t cap,
                                     uint64_t rate, const nts_interval* iv, uint64_t n_iv, uint64_t* n_sampled, nts_sample** out, uint64_t* n_out);
int nts_iv_sites(nts_ctx* ctx, uint32_t n_lists, const nts_sample* const* lists, const uint64_t* n, const nts_sample* target, uint64_t n_target,
                 uint32_t step, uint32_t min_hits, nts_iv_site** out, uint64_t* n_out);

/* ---- the tandem arrays in what the blocks leave out: gap periods ---------------------------------------
 * nts_sample_intervals: nts_bf_sample_intervals without the filter: a k-mer of interval i is sampled when it is valid, lies wholly
 *   inside the interval and h0 <= UINT64_MAX / rate -- nothing is probed, so sequence that one genome alone has is sampled like any
 *   other (rate 1: every k-mer).  The same records in the same order (interval order, then k-mer order), the same clipping,
 *   NTS_EINVAL (rate = 0 included) and NTS_ERANGE, two launches per 2^23 tiles (timers "iv_sample_count", "iv_sample_write"), no
 *   atomic, deterministic; *out released with nts_free().  csrc/nts_iv_sample.inc.
 * nts_iv_periods: recs = n records of ONE list exactly as a sampler returns them (iv does not decrease, off rises strictly within
 *   an iv; checked on the host in one pass: NTS_EINVAL otherwise and for iv >= n_iv).  Within interval i, take the records with
 *   equal h0 in order of off: every one but the first has the lag d = off - its predecessor's off (>= 1); hashes are never paired
 *   across intervals.  out[i] (a host array of n_iv entries, all written): recurring = the records with a lag; period = the lag
 *   held by the most of them, the smallest on a tie; period_hits = how many hold it; first_off = the smallest off - period and
 *   last_off = the largest off over the records whose lag is the period.  All five 0 for an interval without a record or without a
 *   recurrence; n = 0 zeroes out and launches nothing.  Sampling is by hash value, so a k-mer that recurs is sampled at every
 *   recurrence or at none: the lags are exact at any rate.  Three radix sorts, a run-length encoding and two reductions by key on
 *   the context's stream and in its workspace, no atomic, no launch per interval, no floating point: the same input gives the same
 *   bytes (timers "iv_periods_sort", "iv_periods_mode", "iv_periods_extent").  NTS_ERANGE for 2^32 records or intervals or more.
 *   csrc/nts_iv_periods.inc; ntsynt_amd/gaps.py periods, `ntSynt --gap-periods`, `bin/ntsynt_gaps --periods-out`. */
typedef struct
{
  uint32_t recurring, period, period_hits, first_off, last_off;
} nts_iv_period;
int nts_sample_intervals(nts_ctx* ctx, const nts_genome* g, uint32_t k, uint64_t rate, const nts_interval* iv, uint64_t n_iv, uint64_t* n_sampled,
                         nts_sample** out, uint64_t* n_out);
int nts_iv_periods(nts_ctx* ctx, const nts_sample* recs, uint64_t n, uint64_t n_iv, nts_iv_period* out);

/* ---- the tandem arrays grouped into families and found genome-wide: gap families --------------------------
 * Three passes, each linear in its records, all on the context's stream and in its workspace, no atomic, no launch per interval
 * or array, no floating point: the same input gives the same bytes.  csrc/nts_iv_families.inc; ntsynt_amd/gaps.py families,
 * `ntSynt --gap-families`, `bin/ntsynt_gaps --families-out / --family-sites-out`.
 * nts_iv_period_hashes: recs = n records of ONE list exactly as a sampler returns them (the order and the NTS_EINVAL are
 *   nts_iv_periods'); period[i] = interval i's period, 0 = skip the interval (a host array of n_iv entries).  *out = one record per
 *   distinct (iv, h0) that has at least one record whose lag (nts_iv_periods) equals period[iv], off = how many such records there
 *   are, sorted by (iv, h0); (NULL, 0) for none.  Released with nts_free().  Steps 1 - 3 of nts_iv_periods, a scan, a reduction by
 *   key and a selection (timer "iv_phash").  NTS_ERANGE for 2^32 records or intervals or more.
 * nts_iv_families: pairs = n pairs (h0, iv = an array's index; off is ignored, duplicates are allowed), NTS_EINVAL for
 *   iv >= n_arrays.  Two arrays that hold one h0 are joined; family[a] (a host array of n_arrays entries, all written) = the
 *   smallest array index of a's component, a itself for an array without a pair.  *hashes = the distinct h0 ascending,
 *   (*hash_family)[j] = the component of (*hashes)[j] -- every hash belongs to exactly one --, *n_hashes of them; (NULL, NULL, 0)
 *   without a pair.  Both released with nts_free().  Two radix sorts to (h0, iv) order, one lane per pair writes the edge to its
 *   predecessor, a sort and a run-length encoding make the edges unique and another the hashes; the distinct edges -- at most n --
 *   come to the host, where a union-find in which the smaller root wins gives the components (timer "iv_families_join").
 *   NTS_ERANGE for 2^32 pairs or arrays or more.
 * nts_iv_family_sites: occ = ONE genome's records of nts_hset_sample_intervals over whole records (iv = record, off = position; iv
 *   does not decrease, off rises strictly within an iv: checked on the host, NTS_EINVAL otherwise); hashes must ascend strictly
 *   (NTS_EINVAL), hash_family[j] = the family of hashes[j]; an occurrence whose h0 is not among them is dropped.  Within one family
 *   the occurrences in (rec, off) order fall into sites: maximal runs within one record whose consecutive positions differ by at
 *   most `step`; occurrences of other families in between break nothing.  *out = the sites with hits >= min_hits (>= 1: NTS_EINVAL
 *   for 0) sorted by (family, rec, first), *n_out of them; first / last = the first and last position; (NULL, 0) for no site or an
 *   empty input.  Released with nts_free().  A binary search per occurrence, ONE stable radix sort on the family, a scan, a
 *   reduction by key and a selection (timers "iv_family_sites_label", "iv_family_sites_select").  NTS_ERANGE for 2^32 occurrences
 *   or hashes or more. */
typedef struct
{
  uint32_t family, rec, first, last, hits;
} nts_iv_fsite;
int nts_iv_period_hashes(nts_ctx* ctx, const nts_sample* recs, uint64_t n, uint64_t n_iv, const uint32_t* period, nts_sample** out, uint64_t* n_out);
int nts_iv_families(nts_ctx* ctx, const nts_sample* pairs, uint64_t n, uint64_t n_arrays, uint32_t* family, uint64_t** hashes, uint32_t** hash_family,
                    uint64_t* n_hashes);
int nts_iv_family_sites(nts_ctx* ctx, const nts_sample* occ, uint64_t n_occ, const uint64_t* hashes, const uint32_t* hash_family, uint64_t n_hashes,
                        uint32_t step, uint32_t min_hits, nts_iv_fsite** out, uint64_t* n_out);

/* ---- how identical the two sides of a block are, base for base: block identity ----------------------------
 * Two calls, both on the context's stream and in its workspace, no atomic, no launch per interval or segment, no floating point:
 * the same input gives the same bytes.  docs/design/04_16_block_identity.md; ntsynt_amd/assess.py block_identity,
 * `ntSynt --block-identity`, `bin/ntsynt_block_stats --identity-out`.
 * nts_iv_anchor_segments: recs_a / recs_b = ONE genome's records each, exactly as nts_sample_intervals returns them (the order is
 *   checked as nts_iv_periods checks it: NTS_EINVAL, also for a record of A with iv >= n_iv_a).  mate, len_b, flip: host arrays of
 *   n_iv_a entries: mate[i] = the interval of B that interval i of A is paired with (2^32 - 1: none), len_b[i] = that interval's
 *   clipped length, flip[i] = 1 when the two strands differ (anything but 0 or 1: NTS_EINVAL).  An anchor of interval i is a hash
 *   that occurs exactly once among ALL records of A and exactly once among all of B, in i and in mate[i]; x = its off in A, y = its
 *   off in B, or len_b[i] - k - off for a flipped pair (a flipped record with off + k > len_b[i] is no anchor).  Anchors are ordered
 *   by (i, x); two consecutive anchors of one interval make a segment {iv_a = i, x, dx, y_lo = the first one's y, dy, kind}: kind =
 *   NTS_SEG_BACKWARD for dy <= 0, else NTS_SEG_LONG for max(dx, dy) > max_len, else NTS_SEG_OFFBAND for |dy - dx| > band, else
 *   NTS_SEG_CANDIDATE.  *segs = the segments in (iv_a, x) order, *n_segs of them, (NULL, 0) for none; released with nts_free().
 *   anchors_per_iv (a host array of n_iv_a entries, all written) = the anchors of each interval.  A radix sort by hash, a selection,
 *   a radix sort by (iv_a, x), a selection and a run-length encoding (timers "iv_anchors_join", "iv_anchors_segments").  NTS_EINVAL
 *   for k = 0, band outside 1..31, max_len outside 1..65535; NTS_ERANGE before any launch for 2^32 records or more in both lists
 *   together (anchors and segments are fewer) or 2^32 - 1 intervals or more.  csrc/nts_iv_anchors.inc.
 * nts_edit_segments: segs = n_segs segments in iv_a order (NTS_EINVAL otherwise, and for iv_a >= n_iv_a) over the intervals iv_a[i]
 *   of genome g_a and iv_b[i] of g_b -- iv_b[i] is the interval of the MATE of A's interval i; both lists have n_iv_a entries, clipped
 *   to their records as the sampling calls clip; the entries of an interval without a segment are not read.  For a candidate the two
 *   strings are the dx bases of A's interval from x and the dy bases of B's interval from y_lo in the oriented frame: for flip[i] = 1
 *   the reverse complement (A <-> T, C <-> G) of the interval's bases [len - y_lo - dy, len - y_lo).  A candidate that leaves its
 *   interval, has dx or dy outside 1..65535 or |dy - dx| > band is refused with NTS_EINVAL before any launch.  Per segment (dist_out,
 *   n_segs entries, may be NULL): NTS_EDIT_PASSED for kind backward / long / offband, NTS_EDIT_NOT_CANDIDATE for any other kind that
 *   is not a candidate, NTS_EDIT_INVALID when either string holds a base that is not A, C, G or T, else with D the unit-cost edit
 *   distance (Levenshtein) of the two strings NTS_EDIT_OVERBAND when (D + |dy - dx|) / 2 > band, else D -- exact: a distance
 *   restricted to the diagonals -band .. band satisfies the inequality exactly when the unrestricted one does, and then equals it.
 *   per_iv_out[i] (n_iv_a entries, all written): segments = all of interval i's, aligned = those with a D, aligned_a / aligned_b /
 *   edits = their dx / dy / D summed, and the count of each other outcome (too_long: kind long).  One 64-lane wave per segment, a lane
 *   per diagonal, the bases staged through LDS (timer "edit_segments"); a reduction by key (timer "edit_reduce").  NTS_ERANGE
 *   before any launch for 2^32 segments or intervals or more.  csrc/nts_edit.inc. */
#define NTS_SEG_CANDIDATE 0u
#define NTS_SEG_BACKWARD 1u
#define NTS_SEG_LONG 2u
#define NTS_SEG_OFFBAND 3u
#define NTS_EDIT_NOT_CANDIDATE 0xFFFFFFFFu
#define NTS_EDIT_PASSED 0xFFFFFFFEu
#define NTS_EDIT_OVERBAND 0xFFFFFFFDu
#define NTS_EDIT_INVALID 0xFFFFFFFCu
typedef struct
{
  uint32_t iv_a, x, dx, y_lo;
  int32_t dy;
  uint32_t kind;
} nts_iv_segment;
typedef struct
{
  uint64_t aligned_a, aligned_b, edits;
  uint32_t segments, aligned, backward, too_long, offband, invalid, overband, reserved;
} nts_iv_identity;
int nts_iv_anchor_segments(nts_ctx* ctx, const nts_sample* recs_a, uint64_t n_a, const nts_sample* recs_b, uint64_t n_b, const uint32_t* mate,
                           uint64_t n_iv_a, const uint32_t* len_b, const uint8_t* flip, uint32_t k, uint32_t band, uint32_t max_len,
                           nts_iv_segment** segs, uint64_t* n_segs, uint32_t* anchors_per_iv);
int nts_edit_segments(nts_ctx* ctx, const nts_genome* g_a, const nts_genome* g_b, const nts_interval* iv_a, const nts_interval* iv_b,
                      const nts_iv_segment* segs, uint64_t n_segs, uint64_t n_iv_a, const uint8_t* flip, uint32_t band,
                      nts_iv_identity* per_iv_out, uint32_t* dist_out);

/* ---- which edits a segment's distance consists of: block variants -------------------------------------------
 * nts_edit_script: the arguments of nts_edit_segments and its dist_out; all of that call's checks on segments, intervals and flip
 *   are made here too.  For every segment i with a distance D = dist[i] >= 1 the D edits of the CANONICAL script of its two strings A
 *   (n = dx bases) and B (m = dy bases, oriented): with T the unrestricted Levenshtein table, walk from (n, m) to (0, 0) and at (i, j)
 *   take the first that applies -- A[i-1] = B[j-1]: to (i-1, j-1), no edit; T[i-1][j-1] + 1 = T[i][j]: SUB p = i-1, q = j-1;
 *   T[i-1][j] + 1 = T[i][j]: DEL p = i-1, q = j; otherwise INS p = i, q = j-1 -- reported in ascending path order (the reverse of
 *   the walk).  *ops (release with nts_free; NULL for none) holds the scripts one behind the other in segment order, n_ops = the sum
 *   of the distances; first (n_segs + 1 host entries, may be NULL): segment i's ops are first[i] .. first[i+1] - 1.  seg = i; base_a =
 *   the code of A[p] for SUB and DEL, base_b = the code of the oriented (complemented) B[q] for SUB and INS, else 0xFF.
 *   NTS_EINVAL before any launch for a distance on a segment that is no candidate or one with (D + |dy - dx|) / 2 > band (what
 *   nts_edit_segments never returns); NTS_ERANGE for 2^32 edits or more; NTS_EINVAL after the launch, with no ops returned, when some
 *   dist[i] is not the distance of segment i ("dist is not the distance of segment ...") or a string holds a base that is not A, C,
 *   G or T.  A scan and a selection (timer "edit_script_plan"), one 64-lane wave per segment with D >= 1, the furthest-reaching table
 *   of (D + 1) x (2 band + 1) entries in LDS (timer "edit_script").  No atomic, no launch per segment, no floating point: the same
 *   input gives the same bytes.  docs/design/04_17_block_variants.md; csrc/nts_edit_script.inc. */
#define NTS_OP_SUB 1u
#define NTS_OP_DEL 2u
#define NTS_OP_INS 3u
typedef struct
{
  uint32_t seg, p, q;
  uint8_t op, base_a, base_b, pad;
} nts_edit_op;
int nts_edit_script(nts_ctx* ctx, const nts_genome* g_a, const nts_genome* g_b, const nts_interval* iv_a, const nts_interval* iv_b,
                    const nts_iv_segment* segs, uint64_t n_segs, uint64_t n_iv_a, const uint8_t* flip, uint32_t band, const uint32_t* dist,
                    nts_edit_op** ops, uint64_t* n_ops, uint64_t* first);

/* ---- the stretches a 31-diagonal band leaves out: the unrestricted distance up to max_edits edits -----------------
 * nts_edit_wide: the arguments of nts_edit_segments, max_edits = E with 2 band + 1 <= E <= 1023 (NTS_EINVAL otherwise), and dist = that
 *   call's dist_out for the same arguments; all of that call's checks on segments, intervals and flip are made here too.  The WORK SET:
 *   segments of kind offband with |dy - dx| <= E (dist[i] = NTS_EDIT_PASSED) and candidates with dist[i] = NTS_EDIT_OVERBAND.  For a
 *   segment of the work set dist_out[i] = NTS_EDIT_INVALID when either string holds a base that is not A, C, G or T, else with D the
 *   unrestricted unit-cost edit distance of its two strings D when D <= E, else NTS_EDIT_OVERBAND; every other entry is dist[i] (an
 *   offband segment with |dy - dx| > E stays NTS_EDIT_PASSED).  Everything the narrow pass aligns has D <= 2 band + 1 <= E, so after this
 *   call a segment that is neither backward, long nor invalid has a distance exactly when D <= E.  per_iv_out (n_iv_a entries, all
 *   written): the sums of nts_edit_segments over the FINAL results -- aligned = those with a D, offband = kind offband still passed,
 *   overband = every final NTS_EDIT_OVERBAND of either kind.  dist_out (n_segs entries) may be NULL.  NTS_EINVAL before any launch: a
 *   dist[i] that nts_edit_segments does not give a segment of that kind; an offband segment of the work set that leaves its interval
 *   or has dx or dy outside 1..65535.  A selection over a counting iterator keeps the work set (timer "edit_wide_plan"); one 64-lane
 *   wave per kept segment runs the furthest-reaching recurrence over all diagonals, two rows of 2 E + 3 entries in LDS (timer
 *   "edit_wide"); an empty work set launches neither; the sums by nts_edit_segments' reduction (timer "edit_reduce").  On the
 *   context's stream, in its workspace; no atomic, no launch per segment, no floating point: the same input gives the same bytes.
 *   docs/design/04_18_block_identity_wide.md; csrc/nts_edit_wide.inc. */
int nts_edit_wide(nts_ctx* ctx, const nts_genome* g_a, const nts_genome* g_b, const nts_interval* iv_a, const nts_interval* iv_b,
                  const nts_iv_segment* segs, uint64_t n_segs, uint64_t n_iv_a, const uint8_t* flip, uint32_t band, uint32_t max_edits,
                  const uint32_t* dist, nts_iv_identity* per_iv_out, uint32_t* dist_out);

/* ---- which edits the distance of a stretch beyond the band consists of: block wide variants ---------------------
 * nts_edit_wide_script: the arguments of nts_edit_wide, dist = that call's dist_out for the same arguments, and table_budget.  The
 *   SCRIPT SET, decided from dist and the segments alone: dist[i] < NTS_EDIT_INVALID and kind offband, or kind candidate with
 *   D + |dy - dx| > 2 band + 1.  (A candidate with D + |dy - dx| <= 2 band + 1 is nts_edit_script's: it adds nothing here and its
 *   `first` entries are equal.)  For every member the D = dist[i] >= 1 edits of the CANONICAL script nts_edit_script defines, the same
 *   nts_edit_op, in path order, at first[i] .. first[i] + D - 1.  *ops (release with nts_free; NULL for none), n_ops = the members' sum
 *   of D; first (n_segs + 1 host entries, may be NULL; all 0 for an empty script set).  NTS_EINVAL before any launch, with nothing
 *   written: everything nts_edit_segments checks, max_edits outside 2 band + 1 .. 1023; an offband member that leaves its interval or
 *   has dx or dy outside 1..65535; a distance on a kind that is neither candidate nor offband, or D > max_edits, or D < |dy - dx|, or
 *   D = 0 on an offband segment; a
 *   table_budget that is not 0 and below 4 (max_edits + 1)^2 bytes; NTS_ERANGE for 2^32 edits or more.  NTS_EINVAL after the launch,
 *   with no ops returned, when some dist[i] is not the distance of member i ("dist is not the distance of segment ...", the smallest
 *   such index) or a member's string holds a base that is not A, C, G or T.  A member's furthest-reaching table, rows e = 0 .. D as
 *   int32 at e * e + d + e, (D + 1)^2 entries (4 MiB at D = 1023), lies in global memory; the tables of one launch share one block of at
 *   most table_budget bytes (0 = 1 GiB) that is released when the call ends, the host cuts the script set in index order into batches that fit, one launch per batch, and
 *   the result does not depend on the budget.  Two scans and a selection (timer "edit_wide_script_plan"), one 64-lane wave per member
 *   (timer "edit_wide_script"); an empty script set launches nothing.  No atomic, no launch per segment, no floating point: the same
 *   input gives the same bytes.  docs/design/04_19_block_wide_variants.md; csrc/nts_edit_wide_script.inc, csrc/nts_edit_fr_script.inc.
 * nts_edit_wide_script_last_plan: the last such call on this context: members of the script set, bytes of all their tables, batches
 *   (all 0 when nothing was launched); any pointer may be NULL. */
int nts_edit_wide_script(nts_ctx* ctx, const nts_genome* g_a, const nts_genome* g_b, const nts_interval* iv_a, const nts_interval* iv_b,
                         const nts_iv_segment* segs, uint64_t n_segs, uint64_t n_iv_a, const uint8_t* flip, uint32_t band, uint32_t max_edits,
                         const uint32_t* dist, uint64_t table_budget, nts_edit_op** ops, uint64_t* n_ops, uint64_t* first);
int nts_edit_wide_script_last_plan(nts_ctx* ctx, uint64_t* members, uint64_t* table_bytes, uint64_t* batches);

/* ---- how far a block's alignment really continues beyond its first and last anchor: the free-end extension ---------------
 * nts_edit_extend: tasks = n_tasks pairs of strings.  String A of a task is n bases of record rec_a of g_a, read from record position
 *   pos_a forwards (pos_a, pos_a + 1, ...) or, with NTS_EXTEND_A_BACKWARDS, backwards (pos_a, pos_a - 1, ...); string B is m bases of
 *   record rec_b of g_b from pos_b, backwards with NTS_EXTEND_B_BACKWARDS, every base complemented (A <-> T, C <-> G) with
 *   NTS_EXTEND_B_COMPLEMENT.  Both strings are cut before their first base that is not A, C, G or T: valid_a <= n, valid_b <= m.  With
 *   T[i][j] the unrestricted unit-cost edit distance (Levenshtein) of the first i bases of A and the first j of B, penalty = P and
 *   max_edits = E: among the cells 0 <= i <= valid_a, 0 <= j <= valid_b with T[i][j] <= E the one with the largest
 *   S = i + j - P T[i][j]; ties go to the least T, then to the least j - i.  out[t] = {ext_a = i, ext_b = j, edits = T[i][j], valid_a,
 *   valid_b} (n_tasks entries).  One end of the alignment is fixed at (0, 0), the other is free: a match adds 2 to S, a substitution
 *   2 - P, an insertion or deletion 1 - P.  NTS_EINVAL before any launch, with nothing written: P outside 3..255, E outside 1..1023, n
 *   or m above 65535, unknown flag bits, a record index out of range, a string that leaves its record (forwards pos + n > the record's
 *   length, backwards n > pos + 1 or pos at or beyond the record's end; n = 0 reads nothing and is legal at any pos <= the record's
 *   length).  NTS_ERANGE for 2^32 tasks or more.  No task: no launch.  One 64-lane wave per task runs the furthest-reaching rows of
 *   nts_edit_wide without a target corner, two rows of 2 E + 3 entries in LDS, keeps the best entry per lane and stops at the first
 *   row after which no entry can win (timer "edit_extend").  On the context's stream, in its workspace; no atomic, no launch per
 *   task, no floating point: the same input gives the same bytes.  docs/design/04_20_block_ends.md; csrc/nts_edit_extend.inc;
 *   ntsynt_amd/assess.py block_ends, `ntSynt --block-ends`, `bin/ntsynt_block_stats --ends-out`. */
#define NTS_EXTEND_A_BACKWARDS 1u
#define NTS_EXTEND_B_BACKWARDS 2u
#define NTS_EXTEND_B_COMPLEMENT 4u
typedef struct
{
  uint64_t pos_a, pos_b;
  uint32_t rec_a, rec_b, n, m, flags, pad;
} nts_extend_task;
typedef struct
{
  uint32_t ext_a, ext_b, edits, valid_a, valid_b;
} nts_extend_result;
int nts_edit_extend(nts_ctx* ctx, const nts_genome* g_a, const nts_genome* g_b, const nts_extend_task* tasks, uint64_t n_tasks, uint32_t penalty,
                    uint32_t max_edits, nts_extend_result* out);

/* ---- which edits an extended flank consists of: block end variants ---------------------------------------------------
 * nts_edit_extend_script: the tasks of nts_edit_extend and results = what that call wrote for them; valid_a and valid_b are not read.
 *   For task t, A' = the first ext_a bases of its string A as nts_edit_extend reads it (forwards or backwards from pos_a), B' = the
 *   first ext_b bases of its string B as read (forwards or backwards, complemented with NTS_EXTEND_B_COMPLEMENT), D = results[t].edits.
 *   For every task with D >= 1 the D ops of the CANONICAL script of A' and B', exactly as nts_edit_script defines it (walk from
 *   (ext_a, ext_b) to (0, 0), at each cell match first, then SUB, then DEL, else INS; ascending path order), at first[t] ..
 *   first[t + 1] - 1: seg = t, p and q offsets IN THE STRINGS AS READ, base_a = the code of A'[p] for SUB and DEL, base_b = the code
 *   of the complemented-as-read B'[q] for SUB and INS, else 0xFF.  *ops (release with nts_free; NULL for none), n_ops = the sum of D;
 *   first (n_tasks + 1 host entries, may be NULL).  NTS_EINVAL before any launch, with nothing written and the smallest offending
 *   task named: every task check of nts_edit_extend (lengths, flag bits, record index, a string that leaves its record);
 *   ext_a > n or ext_b > m; edits > 1023; edits < |ext_b - ext_a|; edits > max(ext_a, ext_b); a table_budget that is not 0 and below
 *   4 (Dmax + 1)^2 bytes, Dmax the largest edits among the results.  NTS_ERANGE for 2^32 tasks or more, or 2^32 ops or more.
 *   NTS_EINVAL after the launch, with no ops returned ("results is not the extension of task ...", the smallest such index): D edits
 *   do not reach the corner (ext_a, ext_b), or D - 1 already do, or A' or B' holds a base that is not A, C, G or T.  No task, or no
 *   task with D >= 1: no launch, first all 0.  A task's furthest-reaching table, rows e = 0 .. D as int32 at e * e + d + e, (D + 1)^2
 *   entries, lies in global memory; the tables of one launch share one block of at most table_budget bytes (0 = 1 GiB) that is
 *   released when the call ends, the host cuts the tasks with D >= 1 in index order into batches that fit, one launch per batch, and
 *   the result does not depend on the budget.  Two scans and a selection (timer "edit_extend_script_plan"), one 64-lane wave per task
 *   with D >= 1, two rows of 2 Dmax + 3 entries in LDS (timer "edit_extend_script").  No atomic, no launch per task, no floating
 *   point: the same input gives the same bytes.  docs/design/04_21_block_end_variants.md; csrc/nts_edit_extend_script.inc, csrc/nts_edit_fr_script.inc;
 *   ntsynt_amd/assess.py block_ends, `ntSynt --block-end-variants`, `bin/ntsynt_block_stats --end-variants-out`.
 * nts_edit_extend_script_last_plan: the last such call on this context: tasks with D >= 1, bytes of all their tables, batches (all 0
 *   when nothing was launched); any pointer may be NULL. */
int nts_edit_extend_script(nts_ctx* ctx, const nts_genome* g_a, const nts_genome* g_b, const nts_extend_task* tasks, uint64_t n_tasks,
                           const nts_extend_result* results, uint64_t table_budget, nts_edit_op** ops, uint64_t* n_ops, uint64_t* first);
int nts_edit_extend_script_last_plan(nts_ctx* ctx, uint64_t* members, uint64_t* table_bytes, uint64_t* batches);

/* ---- one CIGAR per chain of aligned pieces: block alignments ----------------------------------------------------------
 * nts_cigar_build: pieces = n_pieces pieces in chain order, ops = the ops of all pieces one behind the other, first (n_pieces + 1 host
 *   entries): piece t's ops are first[t] .. first[t + 1] - 1, first[n_pieces] = the number of ops.  A PIECE is two strings of n and m
 *   bases (0 allowed) and its D ops in ascending path order with seg = t and p, q local to the piece: what nts_edit_script,
 *   nts_edit_wide_script and nts_edit_extend_script deliver per segment or task.  Its COLUMNS: from (i, j) = (0, 0) every op gives
 *   g = p - i = q - j >= 0 columns `=` and then one column X for SUB (p < n, q < m; to (p + 1, q + 1)), D for DEL (p < n, q <= m; to
 *   (p + 1, q)) or I for INS (p <= n, q < m; to (p, q + 1)); behind the last op n - i = m - j >= 0 columns `=`.  A piece with
 *   NTS_CIG_REVERSED contributes its columns in reverse order (a flank that was read backwards).  A CHAIN is the concatenation of the
 *   columns of its pieces in the order given; its CIGAR is their run-length encoding: maximal runs of one kind, none of length 0, runs
 *   never merge across chains.  *cigar (release with nts_free; NULL for none), *n_cigar entries len << 4 | code with BAM's codes I 1,
 *   D 2, = 7, X 8, the chains one behind the other; a length may exceed 2^32.  chains (n_chains entries, all written): first and n_cig
 *   locate the chain's entries, eq / x / ins / del are its columns of each kind, len_a = eq + x + del = the sum of n, len_b =
 *   eq + x + ins = the sum of m; a chain without columns is 0 but for first = the entries of all chains before it.  No genome is
 *   read.  NTS_ERANGE before any launch for 2^32 pieces or chains or more, for 2 n_ops + n_pieces >= 2^32, or for lengths that add
 *   up to 2^60 or more.  NTS_EINVAL before any launch, with nothing written and the smallest offending piece named: chain not
 *   nondecreasing or >= n_chains, unknown flag bits, first not nondecreasing from 0.  NTS_EINVAL after the launch, with no CIGAR
 *   returned and chains untouched ("ops of piece ... are no script of its lengths", the smallest such index): an op whose seg is
 *   not its piece's index, an op code outside 1..3, any violation of the column rules.  No piece: no launch.  One lane per op and one
 *   per piece turn ops into (kind, length) atoms, a minimum reduction of the per-lane status (timer "cigar_atoms"); a selection drops
 *   the empty atoms, a reduction by (chain, kind) merges the runs, a reduction by chain and a scan give the records (timer
 *   "cigar_merge").  On the context's stream, in its workspace; no atomic, no launch per piece or chain, no floating point: the same
 *   input gives the same bytes.  docs/design/04_22_block_alignments.md; csrc/nts_cigar.inc; ntsynt_amd/assess.py block_alignments,
 *   `ntSynt --block-paf`, `bin/ntsynt_block_stats --paf-out`. */
#define NTS_CIG_REVERSED 1u
typedef struct
{
  uint32_t chain, n, m, flags;
} nts_cig_piece;
typedef struct
{
  uint64_t first, n_cig, eq, x, ins, del, len_a, len_b;
} nts_cig_chain;
int nts_cigar_build(nts_ctx* ctx, const nts_cig_piece* pieces, uint64_t n_pieces, uint64_t n_chains, const nts_edit_op* ops, const uint64_t* first,
                    uint64_t** cigar, uint64_t* n_cigar, nts_cig_chain* chains);

/* ---- the coordinate map of the chains' CIGARs: block lift --------------------------------------------------------------
 * nts_cigar_lift: cigar = n_cigar entries len << 4 | code (I 1, D 2, = 7, X 8), chains = n_chains records whose first / n_cig locate a
 *   chain's entries and whose len_a / len_b are its bases (what nts_cigar_build returns; entries need not be maximal runs), queries =
 *   n_queries of {chain, side, pos}: pos is an offset on A (side 0) or B (side 1) of the chain, "src"; the answer lies on the other
 *   side, "oth".  An entry consumes A if it is =, X or D and B if it is =, X or I; PA[e] / PB[e] = the bases the chain's entries in
 *   front of e consume.  For pos < len_src the HIT names the one entry e with Psrc[e] <= pos < Psrc[e + 1]: entry = e as an index into
 *   cigar, off = pos - Psrc[e], code = e's code, pos = Poth[e] + off for = and X, and Poth[e] -- the first oth base behind the gap --
 *   for an entry that consumes src only.  For pos = len_src, the end of a half-open interval, the hit is (len_oth, first + n_cig, 0,
 *   0); reserved is 0.  hits: n_queries host entries, written only when the call succeeds.  NTS_ERANGE before any launch for 2^32
 *   entries, chains or queries or more (before any array is read) and for len_a or len_b that add up to 2^63 or more over all chains.
 *   NTS_EINVAL before any launch, the smallest chain named: first not nondecreasing, first + n_cig > n_cigar.  NTS_EINVAL after the
 *   launch, hits untouched: "the entries of chain ... are no CIGAR of its lengths" with the smallest such chain (an entry with a code
 *   outside {1, 2, 7, 8} or of length 0 -- every entry of the array is checked and names the last chain that starts at or in front of
 *   it --, or entries that do not consume len_a and len_b), otherwise "query ... is outside its chain" with the smallest such query
 *   (chain >= n_chains, side > 1, pos > len_src).  No query: the entries are checked, no search is launched, nothing is written.
 *   One exclusive scan over all entries gives the global prefixes of (A bases, B bases), one lane per entry and one per chain check
 *   them, a minimum reduction of the per-lane status (timer "lift_scan"); one lane per query searches its chain's prefixes for the
 *   entry (upper bound, about log2(n_cig) dependent loads) and stores one 32-byte hit, a second minimum reduction (timer
 *   "lift_search").  On the context's stream, in its workspace; no atomic, no launch per chain or query, no floating point: the same
 *   input gives the same bytes.  docs/design/04_23_block_lift.md; csrc/nts_cigar.inc; ntsynt_amd/assess.py block_lift,
 *   `ntSynt --block-lift`, `bin/ntsynt_block_stats --lift-out`. */
typedef struct
{
  uint32_t chain, side;
  uint64_t pos;
} nts_lift_query;
typedef struct
{
  uint64_t pos, entry, off;
  uint32_t code, reserved;
} nts_lift_hit;
int nts_cigar_lift(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains,
                   const nts_lift_query* queries, uint64_t n_queries, nts_lift_hit* hits);

/* ---- the alignment counts of ranges of the chains' CIGARs: lift identity -----------------------------------------------------
 * nts_cigar_lift_stats: cigar, chains as for nts_cigar_lift; ranges = n_ranges of {chain, side, lo, hi}: the bases lo .. hi - 1 of
 *   side A (0) or B (1) of the chain, "src"; valid for chain < n_chains, side <= 1, lo < hi <= len_src.  c_lo / c_hi = the column of
 *   the chain that holds base lo / base hi - 1 (both consume src).  COUNTED are the chain's columns c_lo .. c_hi: columns that
 *   consume the other side only ("oth") are counted strictly between the two, never in front of c_lo or behind c_hi.  eq, x: the = and
 *   X columns among them; src_gap: those that consume src only (D for side 0, I for side 1); oth_gap: those that consume oth only;
 *   src_gaps / oth_gaps: the maximal runs of that kind in the chain's column sequence that hold a counted column (neighbouring
 *   entries of one kind are one run; a run cut by the range's border counts once); [oth_lo, oth_hi): the lifted span -- oth_lo = the
 *   hit position of lo, oth_hi = the hit position of hi - 1, plus 1 if that column is = or X -- so eq + x + src_gap = hi - lo and
 *   eq + x + oth_gap = oth_hi - oth_lo; reserved is 0.  stats: n_ranges host entries, written only when the call succeeds.  Refusals
 *   as for nts_cigar_lift with ranges in the place of queries: NTS_ERANGE before any launch (2^32 entries, chains or ranges or more,
 *   before any array is read; 2^63 bases or more), NTS_EINVAL before any launch with the smallest chain named (first not
 *   nondecreasing, first + n_cig > n_cigar), NTS_EINVAL after the launch with stats untouched: "the entries of chain ... are no CIGAR
 *   of its lengths", otherwise "range ... is outside its chain" with the smallest such range (lo = hi is outside).  No range: the
 *   entries are checked, no search is launched, nothing is written.  ONE exclusive scan over all entries gives the global prefixes of
 *   (A bases, B bases, X columns, D columns, I heads | D heads << 32), nts_cigar_lift's check kernel and a minimum reduction (timer
 *   "lift_stats_scan"); one lane per range makes two upper-bound searches, takes the whole entries between the two as prefix
 *   differences, adds the partial entries at both ends and stores one 64-byte record, a second minimum reduction (timer
 *   "lift_stats_search").  On the context's stream, in its workspace; no atomic, no launch per chain or range, no floating point: the
 *   same input gives the same bytes.  docs/design/04_25_lift_identity.md; csrc/nts_cigar.inc; ntsynt_amd/assess.py
 *   block_lift_identity, `ntSynt --lift-identity / --lift-windows`, `bin/ntsynt_block_stats --lift-identity-out / --lift-windows-out`. */
typedef struct
{
  uint32_t chain, side;
  uint64_t lo, hi;
} nts_lift_range;
typedef struct
{
  uint64_t oth_lo, oth_hi, eq, x, src_gap, oth_gap;
  uint32_t src_gaps, oth_gaps;
  uint64_t reserved;
} nts_lift_stats;
int nts_cigar_lift_stats(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains,
                         const nts_lift_range* ranges, uint64_t n_ranges, nts_lift_stats* stats);

/* ---- one span and its counts per range and pair of chains: the joined lift ------------------------------------------------------
 * nts_cigar_lift_pairs: cigar, chains as for nts_cigar_lift.  links = n_links of {chain, reserved (0), a0, b0}: the chain occupies
 *   [a0, a0 + len_a) on A and [b0, b0 + len_b) on B of a PAIR, in the pair's oriented offsets; pair_first (n_pairs + 1 host entries,
 *   nondecreasing from 0 to n_links) cuts the links into pairs.  The links of one pair ascend without overlap on both sides (equality
 *   allowed), a chain is linked at most once, a chain without entries is not linked; the records need not be ordered by pair.  ranges
 *   = n_ranges of {pair, side, lo, hi}: the bases lo .. hi - 1 of side A (0) or B (1) of the pair, "src"; valid for pair < n_pairs,
 *   side <= 1, lo < hi < 2^63; a range need not touch any chain.  The pair's COLUMNS are those of its linked chains in link order;
 *   between consecutive chains lies an OPEN STRETCH of s0[i + 1] - s1[i] src and o0[i + 1] - o1[i] oth bases that no column covers.
 *   c_lo / c_hi = the first / last column of the pair that holds a src base of [lo, hi); link_lo / link_hi = their links (the links
 *   with s1 > lo and s0 < hi, less those at either end whose chain has no src base).  COUNTED is every column from c_lo to c_hi: the
 *   chains between the two count whole.  src_lo, src_hi: the range clipped to [s0[link_lo], s1[link_hi]); [oth_lo, oth_hi): the lifted
 *   span in the pair's oth offsets, o0 of the end chain plus what nts_cigar_lift_stats makes of that end; eq, x, src_gap, oth_gap: the
 *   counted columns by kind; src_open, oth_open: the bases of the open stretches between link_lo and link_hi; src_gaps, oth_gaps: the
 *   maximal gap runs that hold a counted column -- runs never merge across chains; link_lo, link_hi: indices into links; n_links =
 *   link_hi - link_lo + 1.  A range that touches no chain: every field 0.  eq + x + src_gap + src_open = src_hi - src_lo and eq + x +
 *   oth_gap + oth_open = oth_hi - oth_lo.  stats: n_ranges host entries, written only when the call succeeds.  NTS_ERANGE before any
 *   launch: 2^32 entries, chains, links, pairs or ranges or more (before any array is read), 2^63 bases or more.  NTS_EINVAL before any
 *   launch: nts_cigar_lift's chain checks; pair_first not nondecreasing from 0 to n_links.  NTS_EINVAL after the launch, stats
 *   untouched, the first that applies, the smallest offender named: "the entries of chain ... are no CIGAR of its lengths"; "link ...
 *   is no placement of its chain" (chain >= n_chains, reserved not 0, a chain without entries, a chain with more than one link -- each
 *   of its links --, overlap or disorder against the link in front of it in its pair, a0 + len_a or b0 + len_b >= 2^63); "range ... is
 *   no range of a pair".  No range: the entries and links are checked, no search is launched, nothing is written.  nts_cigar_lift_stats'
 *   scan and check, one lane per link for the placements and the chains' totals, a minimum reduction and one exclusive scan over the
 *   links (timer "lift_pairs_scan"); one lane per range makes two binary searches over its pair's links and two over the end chains'
 *   entries and stores one 128-byte record, a minimum reduction (timer "lift_pairs_search").  On the context's stream, in its
 *   workspace; no atomic, no launch per pair, chain or range, no floating point: the same input gives the same bytes.
 *   docs/design/04_27_lift_joined.md; csrc/nts_cigar.inc; ntsynt_amd/assess.py lift_joined_table, `ntSynt --lift-join`,
 *   `bin/ntsynt_block_stats --lift-joined-out`. */
typedef struct
{
  uint32_t chain, reserved;
  uint64_t a0, b0;
} nts_lift_link;
typedef struct
{
  uint32_t pair, side;
  uint64_t lo, hi;
} nts_pair_range;
typedef struct
{
  uint64_t src_lo, src_hi, oth_lo, oth_hi, eq, x, src_gap, oth_gap, src_open, oth_open;
  uint32_t src_gaps, oth_gaps, link_lo, link_hi, n_links, reserved;
  uint64_t reserved2[3];
} nts_pair_stats;
int nts_cigar_lift_pairs(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains,
                         const nts_lift_link* links, uint64_t n_links, const uint64_t* pair_first, uint64_t n_pairs,
                         const nts_pair_range* ranges, uint64_t n_ranges, nts_pair_stats* stats);

/* ---- one liftover chain per pair of chains: the blocks of a UCSC chain file and their text ---------------------------------------
 * nts_cigar_chain_blocks: cigar, chains, links, pair_first as for nts_cigar_lift_pairs, with its validity rules.  The pair's COLUMNS
 *   are those of its linked chains in link order; between consecutive links lies an open stretch of a0[i + 1] - a1[i] A bases and
 *   b0[i + 1] - b1[i] B bases.  A match column is = or X; a GAP is a D entry (A bases, dt), an I entry (B bases, dq) or an open stretch
 *   (both).  A BLOCK is a maximal run of match columns of the pair with no gap of non-zero width inside it (= next to X is one block;
 *   a block runs across a seam that is closed on both sides).  Block j: size = its columns; dt, dq = the A and B bases of ALL gaps
 *   between it and block j + 1, 0 and 0 for a pair's last block.  Gaps in front of the pair's first match column and behind its last
 *   belong to no block.  pairs[p] (n_pairs host entries, written only when the call succeeds): [a0, a1) x [b0, b1) the liftover chain
 *   in the pair's oriented offsets, from the first match column to behind the last; eq, x its match columns by kind; first_block the
 *   blocks of all pairs in front; n_blocks; a pair without a match column: every field 0.  a1 - a0 = sum size + sum dt, b1 - b0 = sum
 *   size + sum dq, eq + x = sum size, size > 0, dt + dq > 0 for every block but a pair's last.  *blocks (release with nts_free; NULL
 *   for none): *n_blocks records in pair order.  text, text_first both NULL: no text is made.  Otherwise *text (release with
 *   nts_free; NULL for an empty text) holds per block the line "size\tdt\tdq\n", for a pair's last block "size\n", decimal without
 *   padding; pair p's lines are bytes [text_first[p], text_first[p + 1]); text_first: n_pairs + 1 host entries.  NTS_ERANGE before any
 *   launch: 2^32 entries, chains, links or pairs or more (before any array is read), 2^63 bases or more, chain records that hold 2^32
 *   entries or more between them.  NTS_EINVAL before any launch: nts_cigar_lift's chain checks; pair_first not nondecreasing from 0 to
 *   n_links.  After the launch, nothing returned and pairs untouched, the first that applies, the smallest offender named: "the
 *   entries of chain ... are no CIGAR of its lengths"; "link ... is no placement of its chain" (nts_cigar_lift_pairs' conditions,
 *   a0 + len_a or b0 + len_b >= 2^63 among them); NTS_ERANGE for 2^32 blocks or text bytes or more.  No link: the entries are checked,
 *   nothing more is launched, every record is 0 and blocks and text are empty.  nts_cigar_lift's scan and check, nts_cigar_lift_pairs'
 *   two claim kernels, one lane per link, a minimum reduction and one exclusive scan over the links' entry counts (timer
 *   "chain_blocks_scan"); one lane per linked entry finds the heads, one exclusive scan over the linked entries, one lane per block
 *   and one per pair (timer "chain_blocks_emit"); one exclusive scan of the lines' bytes and one lane per aligned 4-byte word of the
 *   text (timer "chain_text").  On the context's stream, in its workspace; no atomic, no launch per pair, chain, link or block, no
 *   floating point: the same input gives the same bytes.  docs/design/04_28_block_chain.md; csrc/nts_cigar.inc; ntsynt_amd/assess.py
 *   block_chains, `ntSynt --block-chain`, `bin/ntsynt_block_stats --chain-out`. */
typedef struct
{
  uint64_t size, dt, dq;
} nts_chain_block;
typedef struct
{
  uint64_t a0, a1, b0, b1, eq, x, first_block;
  uint32_t n_blocks, reserved;
} nts_chain_pair;
int nts_cigar_chain_blocks(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains,
                           const nts_lift_link* links, uint64_t n_links, const uint64_t* pair_first, uint64_t n_pairs, nts_chain_pair* pairs,
                           nts_chain_block** blocks, uint64_t* n_blocks, uint8_t** text, uint64_t* text_first);

/* ---- the cg:Z: and cs:Z: texts of the chains' CIGARs: block alignments with --paf-cs ------------------------------------------
 * nts_cigar_text: cigar, chains as nts_cigar_build returns them (entries need not be maximal runs), but the chains must TILE the
 *   entries: first[0] = 0, first[c + 1] = first[c] + n_cig[c], the last chain ends at n_cigar.  spans = n_chains of {pos_a, pos_b,
 *   rec_a, rec_b, flags}: chain c's len_a target bases are rec_a[pos_a .. pos_a + len_a) of genome a, read forwards; its len_b query
 *   bases are rec_b[pos_b .. pos_b + len_b) of genome b, or with NTS_CIG_B_BACKWARDS rec_b[pos_b], rec_b[pos_b - 1], ..., each
 *   complemented (3 - code): the reverse complement of a PAF `-` record.  spans = NULL (then a = b = NULL): only the cg text is made,
 *   no genome is read, cs and cs_first are ignored.  cg text: per entry the decimal of len and its letter (I, D, =, X).  cs text, short
 *   form: `=` gives `:` and the decimal of len; X gives `*tq` per column (target base, query base as read); D gives `-` and its
 *   target bases; I gives `+` and its query bases as read; lower case acgt, a code that is no base gives n.  *cg / *cs (release with
 *   nts_free; NULL for an empty text): chain c's text is bytes [first[c], first[c + 1]) without a terminator; cg_first / cs_first:
 *   n_chains + 1 host entries.  NTS_ERANGE before any launch: 2^32 entries or chains or more (before any array is read), len_a or
 *   len_b that add up to 2^62 or more.  NTS_EINVAL before any launch, the smallest chain named: chains that do not tile the entries,
 *   unknown flag bits, rec_a / rec_b outside its genome, a span outside its record (pos_a + len_a > rec_len_a; forwards pos_b +
 *   len_b > rec_len_b; backwards pos_b >= rec_len_b or len_b > pos_b + 1; with len_b = 0 only pos_b <= rec_len_b is asked), spans with
 *   a genome missing or genomes without spans.  After the scan: NTS_EINVAL "the entries of chain ... are no CIGAR of its lengths"
 *   (smallest chain; a code outside {1, 2, 7, 8} and a length of 0 included), NTS_ERANGE when either text would hold 2^32 bytes or
 *   more.  A refused call returns no buffer and writes to no caller array.  One exclusive scan over all entries gives the global
 *   prefixes of (A bases, B bases, cg bytes, cs bytes), nts_cigar_lift's check kernel, a minimum reduction and one lane per chain
 *   for the firsts (timer "cigar_text_scan"); one lane per aligned 4-byte word of a text finds the entry of its first byte by an
 *   upper-bound search over the byte prefixes, composes four bytes and stores one dword (timer "cigar_text_emit").  On the
 *   context's stream, in its workspace; no atomic, no launch per chain or entry, no floating point: the same input gives the same
 *   bytes.  docs/design/04_26_block_paf_cs.md; csrc/nts_cigar.inc; ntsynt_amd/assess.py block_alignments(cs=True), `ntSynt --block-paf
 *   --paf-cs`, `bin/ntsynt_block_stats --paf-out F --paf-cs`. */
#define NTS_CIG_B_BACKWARDS 1u
typedef struct
{
  uint64_t pos_a, pos_b;
  uint32_t rec_a, rec_b, flags, pad;
} nts_cig_span;
int nts_cigar_text(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains, const nts_genome* a,
                   const nts_genome* b, const nts_cig_span* spans, uint8_t** cg, uint64_t* cg_first, uint8_t** cs, uint64_t* cs_first);

/* ---- the aligned rows of the chains' CIGARs: the sequence lines of `--block-maf` ------------------------------------------------
 * nts_cigar_rows: cigar, chains, spans, a, b as for nts_cigar_text with spans (the chains TILE the entries; spans, a and b are
 *   required).  A COLUMN is one unit of an entry's length; chain c has eq + x + ins + del columns and two ROWS of that many bytes.
 *   Row A: the target base of the column, rec_a[pos_a ...] read forwards, for =, X and D; `-` for I.  Row B: the query base as read
 *   for =, X and I -- forwards from pos_b, or with NTS_CIG_B_BACKWARDS backwards from pos_b and complemented (3 - code) -- and `-`
 *   for D.  Upper case ACGT; a code that is no base gives N, complemented or not (the codes carry no soft-masking).  *row_a / *row_b
 *   (release with nts_free; NULL for empty rows): chain c's rows are bytes [row_first[c], row_first[c + 1]) of BOTH buffers, without
 *   separator or terminator; row_first: n_chains + 1 host entries.  NTS_ERANGE before any launch: 2^32 entries or chains or more
 *   (before any array is read), len_a or len_b that add up to 2^62 or more.  NTS_EINVAL before any launch, the smallest chain named:
 *   chains that do not tile the entries, unknown flag bits, rec_a / rec_b outside its genome, a span outside its record
 *   (nts_cigar_text's four rules), a NULL genome or NULL spans.  After the scan: NTS_EINVAL "the entries of chain ... are no CIGAR of
 *   its lengths", NTS_ERANGE for 2^32 columns or more.  A refused call returns no buffer and writes to no caller array.  One
 *   exclusive scan over all entries gives the global prefixes of (A bases, B bases, columns), nts_cigar_lift's check kernel, a
 *   minimum reduction and one lane per chain for the firsts (timer "cigar_rows_scan"); ONE kernel makes both rows: one lane per
 *   aligned 4-byte word finds the entry of its first column by one upper-bound search over the column prefix, composes four bytes
 *   per row and stores two dwords (timer "cigar_rows_emit").  On the context's stream, in its workspace; no atomic, no launch per
 *   chain or entry, no floating point: the same input gives the same bytes.  docs/design/04_29_block_maf.md; csrc/nts_cigar.inc;
 *   ntsynt_amd/assess.py block_alignments(maf=True), `ntSynt --block-maf`, `bin/ntsynt_block_stats --maf-out F`. */
int nts_cigar_rows(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains, const nts_genome* a,
                   const nts_genome* b, const nts_cig_span* spans, uint8_t** row_a, uint8_t** row_b, uint64_t* row_first);

/* ---- the padded CIGARs of a reference-anchored (star) multiple alignment: `--block-maf-multi` -------------------------------------
 * nts_cigar_pad: cigar and chains as nts_cigar_build returns them (the chains TILE the entries), every non-empty chain beginning and
 *   ending with an = or X entry (the CORE of a chain: its leading and trailing I and D entries are cut off by the caller), and
 *   at[c] = {group, t0}: the chains of one GROUP (group < n_groups, nondecreasing over the chains) are aligned on their A side to one
 *   reference record, chain c covering its bases [t0, t1 = t0 + len_a).  SLOT p lies in front of reference base p.  An I entry that
 *   precedes base p sits in slot p.  A SITE is a (group, slot) that holds an I entry of a chain of the group; its WIDTH is the longest
 *   of them.  The PADDED CIGAR of chain c is its entries plus entries of BAM code 6 (P, padding: a column that consumes nothing):
 *   behind an own I of length L at a site of width W > L one P of W - L; at every other site p of the group with t0 <= p < t1 one P
 *   of W in front of base p -- between two entries, in front of the chain's first entry for p = t0, or splitting the =, X or D run
 *   that holds bases p - 1 and p in two entries of its code; runs are never merged again across a P; slot t1 is not the chain's.
 *   Out: *padded (release with nts_free; NULL when there is no entry): chain c's padded entries are [pad_first[c], pad_first[c + 1]);
 *   pad_first: n_chains + 1 host entries; the sites ascending by (group, slot): group g's are [site_first[g], site_first[g + 1]) of
 *   *site_pos (the slot, in the reference record's coordinates) and *site_w (its width) (release both with nts_free; NULL when
 *   there is no site); site_first: n_groups + 1 host entries.  No genome is read.  NTS_ERANGE before any launch: 2^32 entries, chains
 *   or groups or more (before any array is read); len_a or len_b that add up to 2^62 or more; t0 + len_a beyond 64 bits; a group
 *   whose chains span 2^32 reference bases or more.  NTS_EINVAL before any launch, the smallest chain named: chains that do not tile
 *   the entries, a group at or beyond n_groups, groups that are not nondecreasing, a first or last entry that is not = or X.  After
 *   the first scan, NTS_EINVAL with the smallest chain named: an entry of code 6 in the input ("is padded already"), and "the entries
 *   of chain ... are no CIGAR of its lengths"; after the second, NTS_ERANGE for 2^32 output entries or more.  A refused call returns
 *   no buffer and writes to no caller array.  The check flags any bad entry of a chain, so a chain with an entry of code 6 and another
 *   fault (a length of 0, say) is reported as "padded already".  PRECONDITION, not checked: no two I entries of one chain are
 *   neighbours (nts_cigar_build merges such runs); two neighbours share a slot and each would be padded to the width, so the chain
 *   would have more columns than col0(t1) - col0(t0).  One exclusive scan over the entries (A bases, B bases, I entries) and
 *   nts_cigar_lift's check; one lane per entry stores an I entry's (group << 32 | slot - the group's smallest t0, length) at its rank,
 *   one radix sort and one reduce_by_key with the maximum give the sites (timer "cigar_pad_sites"); one lane per entry counts what
 *   it becomes from two lower-bound searches over the sites, one exclusive scan, and ONE lane per output entry finds its input entry
 *   by a search over that scan and its piece or P by its rank (timer "cigar_pad_emit").  On the context's stream, in its workspace;
 *   no atomic, no launch per chain, group or site, no floating point: the same input gives the same entries.
 *   docs/design/04_30_block_maf_multi.md; csrc/nts_cigar.inc; ntsynt_amd/assess.py block_multi_mafs. */
typedef struct
{
  uint32_t group;    /* the chain's group: nondecreasing over the chains, below n_groups */
  uint32_t reserved; /* 0 */
  uint64_t t0;       /* the reference base its A side begins at */
} nts_cig_pad_at;
int nts_cigar_pad(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains, const nts_cig_pad_at* at,
                  uint64_t n_groups, uint64_t** padded, uint64_t* pad_first, uint64_t* site_first, uint64_t** site_pos, uint64_t** site_w);

/* nts_cigar_rows_padded: nts_cigar_rows' arguments, results, refusals and kernels (csrc/nts_cigar.inc: k_cig_rows<true>), except that
 *   an entry of code 6 is accepted: it has len columns that are `-` in BOTH rows and consumes no base of either side, so the rows of
 *   a chain nts_cigar_pad has padded are as long as every other row of its group's columns.  nts_cigar_rows itself goes on refusing
 *   code 6.  Timers "cigar_rows_scan" and "cigar_rows_emit". */
int nts_cigar_rows_padded(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains, const nts_genome* a,
                          const nts_genome* b, const nts_cig_span* spans, uint8_t** row_a, uint8_t** row_b, uint64_t* row_first);

/* ---- per-base depth and identity over a star alignment: `--block-conservation` -----------------------------------------------------
 * nts_cigar_depth: cigar, chains (they TILE the entries) and at[c] = {group, t0} as for nts_cigar_pad, but the chains need NOT be
 *   cores, the entries need NOT be maximal runs, and the chains of one group may overlap freely (the call does not know rows).  For a
 *   group g and a reference base p: aligned(g, p) = the chains of g with t0 <= p < t0 + len_a; match(g, p) = those of them in which
 *   p lies in an = entry; gap(g, p) = those in which it lies in a D entry; the mismatches are aligned - match - gap; I entries
 *   consume no reference base and change nothing.  A SEGMENT of group g is a maximal run [start, end) of consecutive reference bases
 *   with aligned > 0 and one constant triple: two = entries separated by an I, two neighbouring X entries, or a chain that ends where
 *   another begins with equal triples on both sides do not split it.
 *   Out: *segs (release with nts_free; NULL when there is no segment): every group's segments ascending by (group, start), group
 *   g's being [seg_first[g], seg_first[g + 1]); seg_first: n_groups + 1 host entries.  No genome is read.  NTS_ERANGE before any
 *   launch: 2^32 entries, chains or groups or more (before any array is read); len_a or len_b that add up to 2^62 or more;
 *   t0 + len_a beyond 64 bits; a group whose chains span 2^32 reference bases or more; a group of 2^20 chains or more (a count would
 *   leave its 21-bit field).  NTS_EINVAL before any launch, the smallest chain named: chains that do not tile the entries, a group at
 *   or beyond n_groups, groups that are not nondecreasing.  After the first scan, NTS_EINVAL with the smallest chain named: "holds
 *   an entry of code 6", and "the entries of chain ... are no CIGAR of its lengths".  A refused call returns no buffer and writes
 *   to no caller array.  One exclusive scan over the entries (A bases, B bases, consuming entries) and nts_cigar_lift's check; one
 *   lane per entry and chain stores n_consuming + n_chains events (the state entered minus the state left, three 21-bit counts in
 *   one word, added modulo 2^64), one radix sort and one reduce_by_key with the sum give the boundaries (timer
 *   "cigar_depth_events"); one inclusive scan gives the states, one lane per boundary marks the heads, one exclusive scan ranks
 *   them, one lane per boundary writes (timer "cigar_depth_emit").  On the context's stream, in its workspace; no atomic, no launch
 *   per chain, group or segment, no floating point: the same input gives the same bytes.
 *   docs/design/04_31_block_conservation.md; csrc/nts_cigar.inc; ntsynt_amd/assess.py block_conservation. */
typedef struct
{
  uint64_t start, end;                  /* reference bases [start, end) of the group's record */
  uint32_t group, aligned, match, gap;  /* mismatches: aligned - match - gap */
} nts_cig_depth_seg;
int nts_cigar_depth(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains, const nts_cig_pad_at* at,
                    uint64_t n_groups, nts_cig_depth_seg** segs, uint64_t* seg_first);

/* ---- variant sites over a star alignment: `--block-variant-sites` --------------------------------------------------------------------
 * nts_cigar_var_bases: nts_cigar_rows' arguments, checks and refusals (entries of code 6 are refused).  With nts_cigar_rows' rows, the
 *   REF bytes of chain c are the bytes of row A at the columns of its X and D entries, in column order, its ALT bytes those of row B at
 *   the columns of its X and I entries: upper case ACGT, N for a code that is no base, B complemented with NTS_CIG_B_BACKWARDS.
 *   Out: *ref and *alt (release with nts_free; NULL for an empty buffer), the chains' bytes one behind the other in chain order; chain
 *   c's are [ref_first[c], ref_first[c + 1]) and [alt_first[c], alt_first[c + 1]): n_chains + 1 host entries each.  Either buffer at
 *   2^32 bytes or more: NTS_ERANGE.  A refused call returns no buffer and writes to no caller array.  One exclusive scan over the
 *   entries (A bases, B bases, events, ref bytes, alt bytes), nts_cigar_lift's check and one lane per chain for either first (timer
 *   "cigar_var_bases_scan"); one lane per aligned 4-byte word of either buffer: an upper-bound search over that buffer's byte prefix,
 *   four bytes through nts_cigar_rows' base fetch, one dword store (timer "cigar_var_bases_emit"; not launched where no chain has an X,
 *   D or I entry).
 * nts_cigar_alleles: cigar, chains (they TILE the entries and are CORES) and at[c] = {group, t0} as for nts_cigar_pad; alt, n_alt: the
 *   alt bytes of nts_cigar_var_bases over ALL chains in chain order (compared as opaque bytes).  An EVENT of chain c: every column of
 *   an X entry at reference base p: (pos p, kind NTS_OP_SUB, len 1, one alt byte); every D entry over [p, p + L): (p, NTS_OP_DEL, L, no
 *   alt byte); every I entry in the slot in front of base p: (p, NTS_OP_INS, L, its L alt bytes).  Two neighbouring D or two
 *   neighbouring I entries of one chain are two events (a precondition, as for nts_cigar_pad, that they do not occur; not checked).
 *   Events of equal (group, pos, kind, len, alt bytes) are one ALLELE; its CARRIERS are their chains, its LEADER the event of the
 *   smallest carrier.  Out: *alleles (release with nts_free; NULL when there is none) ascending by (group, pos, kind, len for DEL and
 *   INS / alt byte for SNV, smallest carrier), group g's being [allele_first[g], allele_first[g + 1]) (n_groups + 1 host entries);
 *   *carriers (nts_free), *n_carriers of them = the events: allele r's are carriers[carrier_first, carrier_first + n_carriers),
 *   ascending; ref_off and alt_off: the leader's offsets into the buffers of nts_cigar_var_bases (a prefix of X + D, of X + I lengths;
 *   ref_off = 0 for INS, alt_off = 0 for DEL).  No genome is read.  Refusals: nts_cigar_pad's, before any launch and behind the first
 *   scan; behind the scan also NTS_EINVAL "alt holds N bytes, the X and I entries of the chains have M" and NTS_ERANGE for 2^32
 *   events or more.  A refused call returns no buffer and writes to no caller array.  One scan as above; one lane per event stores two
 *   key words, two stable radix sorts (timer "cigar_alleles_events"); one lane per sorted event finds its leader -- for an INS by
 *   comparing bytes with the events in front of it in its run of equal (group, pos, len): the one non-linear step, an INS run of r
 *   events costs up to r (r - 1) / 2 comparisons of up to len bytes; exact, no hash --, one stable radix sort by leader, one scan of
 *   the heads, one lane per event to emit (timer "cigar_alleles_emit").  On the context's stream, in its workspace; no atomic, no launch
 *   per chain, group, event or allele, no floating point: the same input gives the same bytes.
 *   docs/design/04_32_block_variant_sites.md; csrc/nts_cigar.inc; ntsynt_amd/assess.py block_variant_sites. */
int nts_cigar_var_bases(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains, const nts_genome* a,
                        const nts_genome* b, const nts_cig_span* spans, uint8_t** ref, uint64_t* ref_first, uint8_t** alt, uint64_t* alt_first);
typedef struct
{
  uint64_t pos, len;                     /* reference base (for INS: the slot in front of it) and length: 1 for NTS_OP_SUB */
  uint64_t ref_off, alt_off;             /* the leader's bytes in nts_cigar_var_bases' buffers */
  uint64_t carrier_first;                /* its carriers: carriers[carrier_first, carrier_first + n_carriers) */
  uint32_t group, kind, n_carriers, reserved;
} nts_cig_allele;
int nts_cigar_alleles(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains, const nts_cig_pad_at* at,
                      uint64_t n_groups, const uint8_t* alt, uint64_t n_alt, nts_cig_allele** alleles, uint64_t* allele_first, uint32_t** carriers,
                      uint64_t* n_carriers);

/* ---- per-column profile and consensus over a star alignment: `--block-consensus` ------------------------------------------------------
 * nts_cigar_profile: cigar, chains (they TILE the entries and are CORES) and at[c] = {group, t0} as for nts_cigar_alleles; ref, n_ref and
 *   alt, n_alt: the ref and alt bytes of nts_cigar_var_bases over ALL chains in chain order (row A at the X and D columns, row B at the
 *   X and I columns).  Chains of one group may overlap freely; the call does not know rows, every count is a count of chains.  The
 *   COLUMNS of group g are (pos, sub): sub = i < W(g, pos) is the i-th column of the slot in front of reference base pos (nts_cigar_pad's
 *   slots and widths), sub = NTS_CIG_PROFILE_REF is base pos itself; ascending (group, pos, sub) is the multi-MAF's column order.  Chain
 *   j COVERS column and slot p when t0 <= p < t0 + len_a (nts_cigar_pad's rule: a foreign site at t0 gives the chain a leading P, the
 *   slot at t1 belongs to no chain).  A reference column: aligned, match, gap as nts_cigar_depth's; n[s], s = A C G T N: the covering
 *   chains with an X there whose alt byte is that letter (any other byte counts under N); match + gap + sum n = aligned; ref: the ref
 *   byte there of the covering chain of smallest index with an X or D (that two chains agree is not checked).  An insertion column
 *   (p, i): aligned = the chains covering slot p; n[s]: those that hold an I entry longer than i in the slot whose i-th byte is s;
 *   gap = aligned - sum n; match = 0; ref = '-'.  CALL: the tallies include the reference row -- on a reference column
 *   t[ref's symbol] = n[that] + match + 1 (a byte outside ACGT: N) and t[-] = gap, on an insertion column t[-] = gap + 1 --; call is one
 *   of "ACGTN-", the symbol of the largest tally; among several the reference's symbol if it is one of them, else the first of A C G T
 *   N -.  EMITTED: every insertion column of every site and every reference column with match < aligned, once each; all others are
 *   unanimous.  Two neighbouring I or D entries of one chain: a precondition, as for nts_cigar_pad, that they do not occur; not
 *   checked.  Split X or D entries give the records of the merged one.
 *   Out: *cols (release with nts_free; NULL when there is none) ascending by (group, pos, sub), group g's being [col_first[g],
 *   col_first[g + 1]) (n_groups + 1 host entries).  No genome is read.  Refusals: nts_cigar_alleles', with the same words, before any
 *   launch and behind the first scan; behind the scan also NTS_EINVAL "alt holds N bytes, the X and I entries of the chains have M",
 *   "ref holds N bytes, the X and D entries of the chains have M" and NTS_ERANGE for 2^32 events or more.  A refused call returns no
 *   buffer and writes to no caller array.  One exclusive scan over the entries (A bases, B bases, events -- one per column of an X, D
 *   or I entry --, ref bytes, alt bytes) and nts_cigar_lift's check; one lane per event stores two key words, two stable radix sorts;
 *   one lane per chain stores where it begins and ends, two radix sorts (timer "cigar_profile_events"); one lane per sorted event
 *   marks the heads, one scan ranks them, one lane per column counts its symbols by lower-bound searches inside its run, its covering
 *   chains by two searches over the chains' sorted ends, and stores the whole record, reserved bytes included (timer
 *   "cigar_profile_emit").  Entries alone: no launch; no event: no launch behind the scan.  On the context's stream, in its workspace;
 *   no atomic, no launch per chain, group, site or column, no floating point: the same input gives the same bytes.
 *   docs/design/04_33_block_consensus.md; csrc/nts_cigar.inc; ntsynt_amd/assess.py block_consensus. */
#define NTS_CIG_PROFILE_REF 0xFFFFFFFFu
typedef struct
{
  uint64_t pos;                          /* reference base; for sub != NTS_CIG_PROFILE_REF the slot in front of it */
  uint32_t group, sub, aligned, match, gap;
  uint32_t n[5];                         /* A C G T N */
  uint8_t ref, call, reserved[6];        /* a letter or '-'; reserved: 0 */
} nts_cig_profile_col;
int nts_cigar_profile(nts_ctx* ctx, const uint64_t* cigar, uint64_t n_cigar, const nts_cig_chain* chains, uint64_t n_chains, const nts_cig_pad_at* at,
                      uint64_t n_groups, const uint8_t* ref, uint64_t n_ref, const uint8_t* alt, uint64_t n_alt, nts_cig_profile_col** cols,
                      uint64_t* col_first);

/* ---- C1-C5: minimizer graph -> collinear chains -----------------------------------------------------
 * replaces ntjoin_utils.read_minimizers' duplicate removal, filter_minimizers and build_graph
 * (call sites bin/ntsynt_synteny.py:607-612, 483, 539) and the path walk of Ntjoin.find_paths
 * (bin/ntsynt_synteny.py:492, 620).
 *
 * nts_graph_build -- on the GPU (radix sorts + scans over all minimizers of all assemblies):
 *   C1  per assembly, keep hashes seen exactly once (over ALL elements given);
 *       then AND with the caller's `keep` mask (refinement rounds: rows C11's position filter);
 *   C2a keep hashes that survive in every assembly; number them 0..nv-1 by ascending hash;
 *   C2b undirected edges between list-adjacent survivors; a "list" is a maximal run of equal
 *       `list_id` inside one assembly (NULL: the record index, i.e. one list per FASTA record);
 *       weight = number of assemblies in which the pair is adjacent.
 * Assemblies are given in the reference's order (descending file name).  Output (host arrays owned by
 * the library; release with nts_graph_free):
 *   v_hash[nv]            surviving hashes, ascending
 *   occ_rec/occ_pos       record and position of vertex v in assembly a at [a*nv + v]
 *   e_u/e_v               endpoints of each distinct edge, in the orientation of its first sighting
 *   e_w                   weight
 *   e_first               sequence number of the first sighting in the reference's traversal order
 *                         (assembly, list, index)
 * Edges are returned in the order ntJoin's dict of dicts iterates them, `[(s, t) for s in edges for t in
 * edges[s]]`: sources by the time they first became a source, then by creation time (bin/ntsynt_synteny.py:573
 * walks the edges in that order, and the order decides which bubbles are removed).
 */
typedef struct
{
  const uint64_t* h1;
  const uint32_t* rec;
  const uint64_t* pos;
  const uint8_t* keep;      /* NULL = keep all */
  const uint32_t* list_id;  /* NULL = rec */
  uint64_t n;
} nts_mxlist;

typedef struct
{
  uint64_t nv;
  uint64_t* v_hash;
  uint32_t* occ_rec;
  uint64_t* occ_pos;
  uint64_t ne;
  uint32_t* e_u;
  uint32_t* e_v;
  uint32_t* e_w;
  uint64_t* e_first;
} nts_graph;
int nts_graph_build(nts_ctx* ctx, uint32_t n_asm, const nts_mxlist* lists, nts_graph* out);
void nts_graph_free(nts_graph* g);

/* Scratch of the graph build (nts_graph_build and nts_engine_add).  The build sorts its items in slices: contiguous ranges of hash
 * values (vertex ids are ranks in hash order), then ranges of the pair keys' smaller end and of the edge order's source rank.  When
 * the slice buffers of all n input minimizers fit the context's budget there is one slice, which holds everything.  Same output
 * however many there are.
 * nts_graph_budget: bytes the per-slice buffers may take (sort keys and values, flags, scans, the sort's temporary storage);
 *     0 = automatic (the default): free device memory plus the allocation cache's free bytes, less a margin, less what the build
 *     keeps n-sized and what its results may grow by.  The input columns, the elements' vertex ids and the results stay n-sized
 *     whatever the budget (docs/design/04_4_graph_stage.md).
 * nts_graph_last_plan: the last build on this context: vertex slices, edge slices (the larger of the pair and order passes; 1 and
 *     1 for a build that fits), library bytes live at its highest beyond those live when the call began, and slices over the budget
 *     (a 32-bit hash prefix, or a bin of the edge passes, that alone does not fit).
 * nts_graph_plan_slices: the host planner.  hist[n_bins] items per bin; cuts[0..*n_slices] (n_bins + 1 entries to hold) with
 *     cuts[0] = 0 and cuts[*n_slices] = n_bins, slice s = bins [cuts[s], cuts[s+1]).  Greedy: a slice takes bins while its items
 *     times bytes_per_elem stay within budget; a bin that alone exceeds it is a slice of its own.  budget 0 is NTS_EINVAL (the
 *     build resolves "automatic" before it plans). */
int nts_graph_budget(nts_ctx* ctx, uint64_t bytes);
int nts_graph_last_plan(nts_ctx* ctx, uint32_t* v_slices, uint32_t* e_slices, uint64_t* scratch_peak_bytes, uint32_t* oversize_slices);
int nts_graph_plan_slices(const uint64_t* hist, uint32_t n_bins, uint64_t bytes_per_elem, uint64_t budget, uint32_t* cuts, uint32_t* n_slices);

/* ---- C1-C9, C11, C12 (erosion): the minimizer graph of a run, resident in HBM across rounds ---------------------------
 * replaces the graph object the reference's stage 3 keeps in igraph / Python dicts (bin/ntsynt_synteny.py:31-32, ntJoin's
 * Ntjoin.graph) and every walk over it; only block tables (a few numbers per synteny block) and the rare-event lists of
 * the bubble rule return to the host.  Kernels and rule-by-rule citations: ntsynt_amd/csrc/nts_dgraph.inc; host driver:
 * ntsynt_amd/synteny_device.py.
 *
 * nts_engine_create(n_asm, ref_asm): assemblies in the reference's order (descending file name, S:34); ref_asm = the one
 *     whose positions orient the paths (ntJoin: the last = lexicographically smallest file).
 * nts_engine_add: build_graph(..., graph=self.graph, black_list=terminals) (S:483, S:612) from minimizer lists resident
 *     in HBM (nts_sketch / nts_mx_allgather results go in without touching the host).  spans == NULL: initial round.
 *     Refinement round (S:476-491, S:256-290): spans[a] = the block interiors of assembly a as composite keys
 *     record * 2^40 + position sorted by `start`, `end_max` = running maximum of the composite ends.
 * nts_engine_bubbles / nts_engine_apply: input and outcome of run_graph_simplification (S:566-590); the rule is order
 *     dependent and touches a handful of edges, it runs on the host over this table.
 * nts_engine_filter: filter_graph_global(_flag_overlaps) (S:292-303, S:491, S:617).
 * nts_engine_erode: refine_graph / erode_edges (S:305-362) over the pairs flagged by the last filter.
 * nts_engine_blocks: find_paths (ntJoin, called at S:492, S:620) by pointer jumping, then find_synteny_blocks,
 *     determine_orientations, check_for_indels, filter_synteny_blocks (S:66-106, synteny_block.py:48-70, S:364-426);
 *     per kept block: first / last vertex, number of minimizers, and per assembly [a * n_blocks + b] the contig, first and
 *     last position and orientation code (0 '+', 1 '-').
 * nts_engine_read: field read-back for tests ("v_hash", "v_alive", "v_rec", "v_pos", "internal", "terminal", "e_u",
 *     "e_v", "e_w", "e_alive", "path_verts", "path_off"). */
typedef struct nts_engine nts_engine;
typedef struct
{
  const uint64_t* start;
  const uint64_t* end_max;
  uint64_t n;
} nts_spans;
typedef struct
{
  uint64_t n_cand;
  uint32_t* cand_edge; /* candidate edges, ascending = the reference's edge order */
  uint64_t n_inc;      /* live edges incident to a candidate's end point */
  uint32_t* inc_edge;
  uint32_t* inc_u;
  uint32_t* inc_v;
  uint32_t* inc_w;
} nts_bubbles;
typedef struct
{
  uint64_t n_blocks;
  uint32_t* first_vid;
  uint32_t* last_vid;
  uint32_t* n_mx;
  uint32_t* rec;       /* [n_asm * n_blocks] */
  uint64_t* first_pos;
  uint64_t* last_pos;
  uint8_t* ori;
  uint64_t stats_paths, stats_unoriented, stats_indel_cuts, stats_small;
} nts_blocks;
int nts_engine_create(nts_ctx* ctx, uint32_t n_asm, uint32_t ref_asm, nts_engine** out);
void nts_engine_free(nts_ctx* ctx, nts_engine* eng);
int nts_engine_size(const nts_engine* eng, uint64_t* nv, uint64_t* ne);
int nts_engine_add(nts_ctx* ctx, nts_engine* eng, const nts_mx* const* lists, const nts_spans* spans, uint64_t* nv, uint64_t* ne);
int nts_engine_bubbles(nts_ctx* ctx, nts_engine* eng, nts_bubbles* out);
void nts_bubbles_free(nts_bubbles* b);
int nts_engine_apply(nts_ctx* ctx, nts_engine* eng, const uint32_t* dead_vertices, uint64_t n_dead, const uint32_t* promote_edges,
                     uint64_t n_promote, uint32_t weight);
int nts_engine_filter(nts_ctx* ctx, nts_engine* eng, uint32_t min_weight, int flag, uint64_t* n_light);
int nts_engine_erode(nts_ctx* ctx, nts_engine* eng, uint32_t k, uint64_t* n_dead_edges);
int nts_engine_blocks(nts_ctx* ctx, nts_engine* eng, int64_t bp, double m_percent, uint32_t min_mx, nts_blocks* out);
void nts_blocks_free(nts_blocks* b);
int nts_engine_paths(const nts_engine* eng, uint64_t* n_paths, uint64_t* n_verts);
int nts_engine_read(nts_ctx* ctx, const nts_engine* eng, const char* field, void* dst, uint64_t bytes);

/* ---- block-level rules over flat tables (host side, no GPU work): what is left of the reference's per-object Python once the
 * graph lives in HBM -- sequential where the reference's rule is order dependent.
 * nts_bubble_rule : run_graph_simplification (bin/ntsynt_synteny.py:566-590) over nts_engine_bubbles' table; doomed[i] /
 *     promoted[i] (caller-allocated, n_cand entries) = middle vertex and candidate edge of the i-th bubble, *n_out of them.
 * nts_blocks_merge: merge_collinear_blocks (S:428-472) in place over blocks sorted like SyntenyBlock.__lt__; tables are
 *     [a * n + b]; ori 0 '+' 1 '-'; reason 0 None, 1 id_change, 2 ori_change, 3 inconsistent_order, 4 indel, 5 merge.
 * nts_blocks_text : get_block_string (bin/synteny_block.py:72-85) for a table: blocks shorter than z in any assembly skipped,
 *     the others numbered from 0, rows in out_order; `reason` != NULL adds the verbose column.  names = NUL-separated
 *     strings: the G assembly names, then every assembly's contig names; contig_base[a] = index of assembly a's first contig
 *     among the contig names.  *text is released with nts_free. */
int nts_bubble_rule(uint64_t n_cand, const uint32_t* cand_edge, uint64_t n_inc, const uint32_t* inc_edge, const uint32_t* inc_u,
                    const uint32_t* inc_v, const uint32_t* inc_w, uint32_t wmax, uint32_t* doomed, uint32_t* promoted, uint64_t* n_out);
int nts_blocks_merge(uint32_t n_asm, uint64_t n, int64_t k, int64_t bp, int64_t collinear_merge, uint32_t* rec, int64_t* first,
                     int64_t* last, uint8_t* ori, int64_t* n_mx, uint8_t* reason, uint64_t* n_out, uint64_t* n_merged);
int nts_blocks_text(uint32_t n_asm, uint64_t n, int64_t k, int64_t z, const uint32_t* out_order, const char* names, uint64_t names_bytes,
                    const uint64_t* contig_base, const uint32_t* rec, const int64_t* first, const int64_t* last, const uint8_t* ori,
                    const int64_t* n_mx, const uint8_t* reason, char** text, uint64_t* text_bytes);

/* Host-side helper (no GPU work): connected components of an undirected graph given as edge arrays
 * that are simple paths (two degree-1 ends, everything else degree 2, at least 2 vertices) -- what
 * Ntjoin.find_paths keeps.  Path i is verts[off[i] .. off[i+1]); each path starts at its end with the
 * smaller vertex id.  Paths are listed by ascending first vertex id.  Release with nts_free(). */
int nts_walk_chains(uint64_t nv, uint64_t ne, const uint32_t* e_u, const uint32_t* e_v,
                    uint64_t** off, uint32_t** verts, uint64_t* n_paths);

/* The same walk on the engine's own arrays: 64-bit edge ends, an optional liveness byte per edge (NULL = all
 * live) and an optional per-vertex key: with a key, each path is written starting at the end with the smaller
 * key (row C5: ntJoin's find_paths, called at bin/ntsynt_synteny.py:620, starts a path at the end with the
 * smaller position in the reference assembly) while the paths keep the order above (ascending smaller-id end). */
int nts_walk_paths(uint64_t nv, uint64_t ne, const int64_t* e_u, const int64_t* e_v, const uint8_t* e_alive,
                   const int64_t* key, uint64_t** off, int64_t** verts, uint64_t* n_paths);

/* Host-side helper (host threads): dst[i] = src[i] as a 64-bit integer, src holding 32-bit (src_bytes 4) or 64-bit (8)
 * unsigned values -- how a caller that keeps everything in int64 (the Python engine) takes over nts_graph's arrays. */
int nts_to_i64(const void* src, uint32_t src_bytes, uint64_t n, int64_t* dst);

/* Host-side helper: deg[v] = number of live edge ends at v, saturating at 255 (bubble detection asks
 * "degree 3", bin/ntsynt_synteny.py:548-590; path ends ask "degree 1"). */
int nts_edge_degrees(uint64_t nv, uint64_t ne, const int64_t* e_u, const int64_t* e_v, const uint8_t* e_alive,
                     uint8_t* deg);

/* Host-side helper (no GPU work, host threads): one pass over the paths of a round -- path i is
 * verts[off[i] .. off[i+1]) -- against the per-assembly vertex tables v_rec / v_pos ([a*nv + v]):
 *   start[i]          index into verts of the first vertex kept: a path whose contig changes in any assembly
 *                     keeps only its last run (bin/ntsynt_synteny.py:71-77);
 *   n_up[a*n_paths+i] steps of the kept run along which the position in assembly a rises -- the orientation
 *                     rule's input (bin/synteny_block.py:48-65);
 *   over[j]           1 where the distance from verts[j] to verts[j+1] differs between two assemblies by more
 *                     than bp (indel split, bin/ntsynt_synteny.py:364-409); 0 outside kept runs.
 * All outputs are caller-allocated (n_paths, n_asm*n_paths, off[n_paths] elements). */
int nts_path_scan(uint32_t n_asm, uint64_t nv, const int64_t* v_rec, const int64_t* v_pos, uint64_t n_paths,
                  const uint64_t* off, const int64_t* verts, int64_t bp, uint64_t* start, uint64_t* n_up,
                  uint8_t* over);

/* ---- host-side I/O (no GPU work) ---------------------------------------------------------------------
 * nts_fasta_read: plain or gzip FASTA, single- or multi-line, LF or CRLF -> concatenated bases + record table +
 *   record ids (header up to the first whitespace, NUL-separated) + the `samtools faidx` columns; NTS_EFORMAT for a
 *   non-empty file that does not start with a '>' header (FASTQ is not accepted).  Replaces
 *   btllib::SeqReader(LONG_MODE) record streaming (src/ntsynt_make_common_bf.cpp:32-36) and rule faidx (smk:48-53).
 * nts_write_indexlr_tsv: `indexlr --long --pos [--seq]` text (smk:81-85): "id\thash:pos[:KMER] ...\n" per record;
 *   minimizers given in (record, position) order as nts_mx_download returns them. */
typedef struct
{
  uint8_t* seq;
  uint64_t n;
  uint32_t n_rec;
  uint64_t* rec_off;
  uint64_t* rec_len;
  char* names;
  uint64_t names_bytes;
  uint64_t* fai_offset;
  uint32_t* fai_linebases;
  uint32_t* fai_linewidth;
} nts_fasta;
int nts_fasta_read(const char* path, nts_fasta* out);
/* The same ingest with the parse on the GPU: the file's bytes (plain: mapped; .gz: inflated on the
 * host) go to HBM through pinned staging, kernels find the header lines, drop line ends, compact and encode the bases into
 * a resident genome and produce the record table and the faidx columns; the host reads only the header lines.  `meta` as
 * nts_fasta_read fills it, except seq == NULL (the bases never exist on the host; nts_mx_kmers serves `--seq` output).
 * Same rules as nts_fasta_read (white space at either end of a sequence line is dropped, inside a line it is an invalid base).
 * nts_ingest_trim: gives back what the ingest keeps between files -- the image of the largest file read so far (as large as
 * that file, in HBM) and the pinned staging lanes -- once the last genome of a run is resident. */
int nts_genome_from_fasta(nts_ctx* ctx, const char* path, nts_genome** out, nts_fasta* meta);
int nts_ingest_trim(nts_ctx* ctx);
/* the Bloom build's bucket arrays (24 GB at 3 Gbp) back to the library's allocation cache once the last filter of a run is made (rules
 * indexlr and ntsynt_synteny build none: bin/ntsynt_run_pipeline.smk:74-103): later allocations are cut from them; the next build, if
 * there is one, takes them up again */
int nts_bf_build_trim(nts_ctx* ctx);
/* nts_write_indexlr_tsv for records whose bases are not on the host (fa->seq == NULL): `kmers` = nts_mx_kmers' output, or
 * NULL without --seq */
int nts_write_indexlr_tsv_kmers(const char* path, const nts_fasta* fa, const uint64_t* h1, const uint32_t* rec, const uint64_t* pos,
                                uint64_t n, uint32_t k, const uint8_t* kmers);
void nts_fasta_free(nts_fasta* f);
/* nts_read_indexlr_tsv: ntJoin's read_minimizers on an `indexlr --long --pos [--seq]` file -- the input of the reference's stage 3
 * (bin/ntsynt_run.py:12 FILES, bin/ntsynt_synteny.py:607-609; file format: rule indexlr, smk:74-85): per line the record id and its
 * tokens "hash:pos[:KMER]".  Out: the ids of all lines (NUL-separated, in file order), and per token the printed hash, the position
 * and the number of its line, in file order.  NTS_EFORMAT for a token without a position.  Released with nts_mx_tsv_free. */
typedef struct
{
  uint64_t n_lines;
  char* names;
  uint64_t names_bytes;
  uint64_t n;
  uint64_t* h1;
  uint64_t* pos;
  uint32_t* line;
} nts_mx_tsv;
int nts_read_indexlr_tsv(const char* path, nts_mx_tsv* out);
void nts_mx_tsv_free(nts_mx_tsv* t);
int nts_write_indexlr_tsv(const char* path, const nts_fasta* fa, const uint64_t* h1, const uint32_t* rec, const uint64_t* pos,
                          uint64_t n, uint32_t k, int with_seq);

void nts_free(void* p);

#ifdef __cplusplus
}
#endif
#endif

/* include/lra_hip.h -- C ABI of liblra_hip.so: the MI355X (gfx950) replacement for the
 * per-read alignment hot path of ChaissonLab/LRA (MapRead.h:153-263 and what it calls).
 *
 * The reference has no FFI seam: every stage is a C++ function template #included into
 * lra.cpp.  Each entry point below replaces ONE of those functions for a whole BATCH of
 * reads / sub-problems (the GPU needs thousands at once), and cites the reference
 * function it replaces.  A maintainer binds them from MapRead.h as shown in
 * INTEGRATION.md.
 *
 * Conventions
 *   - plain C types only; no torch / STL types cross the boundary;
 *   - pointers named d_* are DEVICE (HBM) pointers, h_* are host pointers;
 *   - every call is asynchronous on the context's HIP stream (lra_ctx_set_stream) unless
 *     it says "synchronous"; the caller synchronises the stream before reading results;
 *   - return value: 0 = ok, negative = error (lra_ctx_last_error gives the text); the
 *     library never calls exit() (the reference exit(1)s, lra.cpp:623-640);
 *   - per-item `status` words report conditions that are undefined behaviour or an
 *     endless loop in the reference (so no parity is defined for them).
 *
 * Lifetime of results.  Output arrays marked "context-owned" live in growable buffers of
 * the context and stay valid until a later call reuses their buffer; a buffer that has to
 * grow is freed and allocated again (contents are not preserved).  Which calls share
 * buffers (copy a result out with lra_copy_device if it has to survive one of them):
 *   - every sparse DP call (lra_sparse_dp_batch, lra_sparse_dp_boxes_batch, and the ones
 *     inside lra_local_refine_batch / _highacc_batch) overwrites the previous sparse DP's
 *     lra_chain_result;
 *   - lra_indel_refine_batch and lra_calculate_statistics_batch keep their temporaries in
 *     the sparse DP's arena: a chain result does not survive them either way, their own
 *     results (refined blocks, counters, CIGAR runs) have buffers of their own;
 *   - lra_indel_refine_batch's d_status lives in scratch the statistics stage reuses;
 *   - lra_filter_chains_batch shares its buffer with lra_split_chains_batch,
 *     lra_refine_clusters_batch with lra_refine_splitchain_batch;
 *   - a lra_map_reads_*_batch call invalidates every result of the call before it (and a
 *     pending two-call lra_map_records text); lra_map_snapshot / lra_map_pack take what the
 *     record stage needs out of the context first;
 *   - lra_map_records_device, _bgzf and _bam share the record stage's buffers (the text or the
 *     BAM record stream of the last call only); _bam also calls lra_bam_cigar_batch,
 *     lra_bam_pack_seq_batch and lra_bam_phred_batch, whose results have buffers of their own.
 * Output: the record stage writes SAM / PAF / BED / pairwise text, the same text as BGZF
 * members (lra_map_records_device_bgzf) and BAM records (lra_map_records_device_bam with
 * lra_bam_header), the last two made on the device before anything crosses to the host.
 * The two drivers are the tested orderings of these calls.
 */
#ifndef LRA_HIP_H_
#define LRA_HIP_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lra_ctx lra_ctx;

#define LRA_OK 0
#define LRA_ERR_INVALID (-1)
#define LRA_ERR_HIP (-2)
#define LRA_ERR_NOMEM (-3)

/* per-item status bits */
#define LRA_ST_OOB_SLOT 1      /* reference would index outside its matrices            */
#define LRA_ST_NO_TERMINATION 2 /* reference trace back would loop forever              */
#define LRA_ST_RANGE 4         /* problem too large for the 32-bit device score range   */
#define LRA_ST_CAPACITY 8      /* caller-provided output capacity exceeded              */
#define LRA_ST_REJECTED 16     /* the reference drops the item itself (e.g. a cluster spanning two chromosomes) */
#define LRA_ST_UNSUPPORTED 32  /* the read takes a branch of the reference this library has not built (it gets no record) */
#define LRA_ST_DEFERRED 64     /* scheduling, not an error: with opts.defer_seed_matches the read was handed back unmapped (the caller maps it in a later batch of
                                * its own kind; no record is written for it here).  Also used inside lra_map_reads_lowacc_batch for opts.defer_matches (never in a result) */

/* ---- context ---------------------------------------------------------------------- */
int lra_ctx_create(int device_id, lra_ctx** out);
void lra_ctx_destroy(lra_ctx* ctx);
/* (ABI 9) Frees the context's growable WORK buffers -- its own, its companion contexts' (a second pass, the back half and the handover sets of two-stage batches) -- and
 * keeps everything loaded into it (genome, chromosome table, both indexes).  The buffers grow to what the largest batch needed and are kept
 * from call to call (a batch of 28672 reads of 30 kb holds ~250 GB of them); a caller that wants the memory back -- after a call failed with LRA_ERR_NOMEM and before it
 * retries with a smaller batch, or between jobs -- calls this.  No batch may be in flight on the context (LRA_ERR_INVALID while a batch sits between the halves of a
 * two-stage batch), and every result of an earlier call (lra_map_result and friends: device pointers into these buffers) is void afterwards.  The reference this
 * boundary replaces has no counterpart: its buffers are the process heap's.  Returns the bytes freed through *bytes (may be NULL).                                  */
int lra_ctx_release_buffers(lra_ctx* ctx, uint64_t* bytes);
/* stream = a hipStream_t (NULL = the default stream).  All later calls launch on it. */
int lra_ctx_set_stream(lra_ctx* ctx, void* stream);
const char* lra_ctx_last_error(lra_ctx* ctx);
/* lra align -a, "Query all positions in a read, not just minimizers" (lra.cpp:182-184, opts.storeAll): with the switch on, the drivers
 * (lra_map_reads_lowacc_batch, lra_map_reads_lowacc_front, lra_map_reads_highacc_batch, lra_map_reads_host) sketch each read with w = 1 -- MapRead.h:172-176
 * copies the options, sets allOpts.globalW = 1 on the copy and calls StoreMinimizers(read, globalK, 1) -- and keep opts.globalW for everything after the sketch
 * (the high-accuracy RefineBtwnClusters_chain's W, Map_highacc.h:466-468).  A context setting rather than a field of lra_map_opts, which callers allocate and
 * the presets write in full.  Off when the context is made.  on must be 0 or 1; a NULL ctx or another value is LRA_ERR_INVALID.
 * lra_ctx_store_all returns the switch (0 / 1), or LRA_ERR_INVALID for a NULL ctx.                                                                                  */
int lra_ctx_set_store_all(lra_ctx* ctx, int on);
int lra_ctx_store_all(lra_ctx* ctx);
/* opts.svsigLen (Options.h:70; `-SV LEN PATH`, lra.cpp:64): the net gap length above which the record stage (LRA_PACK_SVSIG) emits an SV signature.
 * A context setting, like the one above: lra_map_opts and lra_map_result stay as they are.  Default 25; a negative len is LRA_ERR_INVALID.
 * lra_ctx_svsig_len returns the value, or LRA_ERR_INVALID for a NULL ctx.                                                                     */
int lra_ctx_set_svsig_len(lra_ctx* ctx, int len);
int lra_ctx_svsig_len(lra_ctx* ctx);
/* ABI version of the loaded library (tests check it against this header). */
int lra_abi_version(void);
#define LRA_ABI_VERSION 9   /* 9: lra_ctx_release_buffers; later, additively (no struct or signature changed): lra_aog_class_of_batch; lra_ctx_set_store_all, lra_ctx_store_all; SV signatures: lra_sv_signatures_batch, lra_ctx_set_svsig_len, lra_ctx_svsig_len, lra_map_svsig_host, lra_map_svsig; SAM / BAM input: lra_reads_set_flag_remove, lra_reads_set_passthrough, lra_reads_batch_tags, lra_map_records_tags, lra_map_records_host_tags, lra_bgzf_inflate_batch, lra_bgzf_inflate_host; the genome reader: lra_genome_open, _read_host, _read_device, _info, _names, _host_seq, _device_seq, _install, _last_error, _set_device_chunk, _close; 8: lra_map_opts_apply_local_index, lra_ctx_local_index_params, lra_ctx_load_local_index (the .gli file's k / w / window override the options', as glIndex.Read does); 7: lra_sort_pairs_batch;  2: lra_map_opts.defer_matches, lra_map_counters.n_deferred_reads; 3: lra_map_opts.flagged_unaligned, lra_map_counters.n_flagged_reads, lra_map_host_flagged; 4: lra_reads_last_error, a corrupt FASTQ record is LRA_ERR_INVALID; lra_map_opts.defer_seed_matches; 5: lra_seed_prefetch, lra_ctx_adopt_seed, lra_map_reads_lowacc_front / _back, lra_map_back_release; 6: a failed front half hands over an error batch (one back call per front call), separate n_handed_back_reads counter, lra_map_host_trim */

/* Convenience for hosts without their own HIP binding: synchronous device->host copy on the
 * context's stream (a C++ host would call hipMemcpy itself).                                */
int lra_copy_to_host(lra_ctx* ctx, void* h_dst, const void* d_src, uint64_t bytes);

/* Asynchronous device->device copy on the context's stream (e.g. out of context-owned result
 * arrays into caller-owned memory before the next call recycles them).                        */
int lra_copy_device(lra_ctx* ctx, void* d_dst, const void* d_src, uint64_t bytes);

/* Per-kernel device timing (HIP events on the context's stream around every kernel the
 * library launches).  Off by default.  lra_ctx_timing_get synchronises the stream and returns
 * the accumulated milliseconds and launch count of the named kernel since the last reset
 * (names: see DESIGN.md "kernels"); returns LRA_ERR_INVALID for an unknown name.            */
int lra_ctx_timing_enable(lra_ctx* ctx, int on);
int lra_ctx_timing_reset(lra_ctx* ctx);
int lra_ctx_timing_get(lra_ctx* ctx, const char* name, double* total_ms, int* launches);

/* ---- reference data (replicated per GPU) ---------------------------------------------
 * Genome: the concatenated upper-case chromosome bytes, chromosome c at global offset
 * header.pos[c] (Genome.h:59-68, Genome::Read :115-138 upper-cases).  Replaces the role of
 * Genome::seqs / GlobalIndexToSeq (Genome.h:106-112) for the device side.  Synchronous copy. */
int lra_ctx_load_genome(lra_ctx* ctx, const char* h_seq, uint64_t len);
/* Global minimizer index = the payload of `ref.mms` (MMIndex.h:402-424): n GenomeTuples
 * sorted by (t & 2^63-1), passed as two host arrays (t, pos).  Replaces `genomemm`
 * (MapRead.h:153).  Synchronous copy.                                                       */
int lra_ctx_load_global_index(lra_ctx* ctx, const uint64_t* h_key, const uint32_t* h_pos, uint64_t n);
/* The same two from device memory / built on the device:
 *   lra_ctx_load_genome_device  copies len bytes from a device buffer.
 *   lra_ctx_build_global_index  `lra index` on the loaded genome: StoreIndex (MMIndex.h:286-400) -- per chromosome
 *       StoreMinimizers<GenomeTuple,Tuple>(seq, len, k, w) (MinCount.h:8-179), sort by masked key, keys occurring more than
 *       max_freq (opts.globalMaxFreq) times dropped, then at most n_per_window (opts.NumOfminimizersPerWindow) entries per window of
 *       winsize (opts.globalWinsize) bases in CountSort's order (:258-283: frequency ascending, sorted position descending) -- and
 *       installs the result as the context's global index.  Index-time presets (lra.cpp:884-911): -ONT / -CCS 17, 10, 150, 15, 1;
 *       -CLR 15, 10, 250, 12, 1; -CONTIG 19, 10, 30, 20, 1.  h_chrom_pos: n_chrom + 1 cumulative starts (Genome::header.pos).
 *       The entries and their key order are StoreIndex's; equal keys keep their emission order (the reference: libstdc++'s std::sort
 *       permutation), which also decides between two equal-key candidates inside one window.  *status = LRA_ST_OOB_SLOT when the
 *       reference would index winCount out of range (:359-366).  Synchronous.
 *   lra_ctx_global_index        the context's index as device arrays (for lra_write_mms after a copy to the host).                 */
int lra_ctx_load_genome_device(lra_ctx* ctx, const char* d_seq, uint64_t len);
int lra_ctx_build_global_index(lra_ctx* ctx, const uint64_t* h_chrom_pos, int n_chrom, int k, int w, int max_freq, int winsize, int n_per_window,
                               uint64_t* n_minimizers, uint64_t* n_index, int* status);
int lra_ctx_global_index(lra_ctx* ctx, const uint64_t** d_key, const uint32_t** d_pos, uint64_t* n);
/* Index files (host arrays, host I/O), byte layouts of the reference:
 *   .mms  WriteIndex / ReadIndex (MMIndex.h:402-424; Header::Write / Read Genome.h:59-84): int64 n; int32 globalK; int32 nChrom; per
 *         chromosome int32 nameLen + name bytes; uint64 pos[nChrom + 1]; n GenomeTuples of 16 bytes {uint64 t; uint32 pos; 4 bytes of
 *         padding (zeros here)}.  lra_read_mms: first call with key == NULL returns *n, *globalK, *n_chrom, *names_len (bytes for the
 *         names, each NUL-terminated); the second call fills names, chrom_pos[n_chrom + 1], key[n], pos[n].
 *   .gli  LocalIndex::Write / Read (MMIndex.h:138-173): int32 k, w, localIndexWindow, nRegions = n_windows + 1; uint64 seqOffsets[nRegions];
 *         uint64 tupleBoundaries[nRegions]; uint64 nMin; nMin LocalTuples (uint32: t in the low 20 bits, pos in the high 12).
 *         lra_read_gli: first call with seq_offsets == NULL returns the sizes.  The filling calls of both readers take the values the sizing call
 *         left in *n / *n_chrom / *names_len (*n_windows / *n_tuples) as the capacities of the caller's buffers and fail when the file holds more.      */
int lra_write_mms(const char* path, int globalK, const char* const* chrom_names, const uint64_t* chrom_pos, int n_chrom, const uint64_t* key,
                  const uint32_t* pos, uint64_t n);
int lra_read_mms(const char* path, int* globalK, uint64_t* n, int* n_chrom, uint64_t* names_len, char* names, uint64_t* chrom_pos, uint64_t* key,
                 uint32_t* pos);
int lra_write_gli(const char* path, int k, int w, int window, uint64_t n_windows, const uint64_t* seq_offsets, const uint64_t* tuple_bnd,
                  const uint32_t* tuples);
int lra_read_gli(const char* path, int* k, int* w, int* window, uint64_t* n_windows, uint64_t* n_tuples, uint64_t* seq_offsets, uint64_t* tuple_bnd,
                 uint32_t* tuples);

/* ---- a1-a4: tier-1 seeding of a read batch ---------------------------------------------
 * Replaces, per read (MapRead.h:169-203):
 *   StoreMinimizers<GenomeTuple,Tuple>(read.seq, read.length, k, w, readmm, true)  MinCount.h:8
 *   sort(readmm.begin(), readmm.end())                                            MapRead.h:185
 *   CompareLists<GenomeTuple,Tuple>(readmm, genomemm, allMatches, opts, true)     CompareLists.h:9
 *   SeparateMatchesByStrand(read, genome, k, allMatches, forMatches, revMatches)  MapRead.h:109
 * Input: n_reads upper-case ASCII reads concatenated in d_seq, read r = bytes
 * [d_read_off[r], d_read_off[r+1]).  k = opts.globalK, w = opts.globalW (1 for lra align -a,
 * lra_ctx_set_store_all: every position whose k-mer is free of non-ACGT bytes, position-parallel
 * over the batch), max_freq = opts.globalMaxFreq.
 * Output (device arrays owned by the context, valid until the next lra_seed_batch call on
 * it; CSR by read):
 *   d_mm_*     readmm after the sort (t with the strand flag in bit 63, pos)
 *   d_match_*  allMatches in the reference's order: (index into the read's readmm,
 *              index into the global index) per pair
 *   d_sep_*    forMatches then revMatches of each read (read pos, genome pos of each pair),
 *              d_n_forward[r] = forMatches.size()
 * Synchronous: returns after the results are complete (two host round trips size the
 * outputs).
 * Lifetime of OTHER results on the same context: the sketch is staged in the context's sparse-DP
 * arena -- the allocation that also holds the IndelRefine / CalculateStatistics arrays of the last
 * lra_map_result.  A stage call on a context (this one, lra_sparse_dp_batch, ...) therefore ends the
 * lifetime of the map result of an earlier batch call on THAT context: take what is needed from it
 * first (lra_map_pack / lra_map_snapshot / lra_map_records), or seed on another context
 * (lra_seed_prefetch).                                                                       */
typedef struct lra_seed_result {
  int32_t n_reads;
  uint64_t n_minimizers, n_matches;
  const uint64_t* d_mm_off;    /* [n_reads+1] */
  const uint64_t* d_mm_key;    /* [n_minimizers] */
  const uint32_t* d_mm_pos;    /* [n_minimizers] */
  const uint64_t* d_match_off; /* [n_reads+1] */
  const uint32_t* d_match_qi;  /* [n_matches] */
  const uint32_t* d_match_ti;  /* [n_matches] */
  const uint32_t* d_n_forward; /* [n_reads] */
  const uint32_t* d_sep_qpos;  /* [n_matches] */
  const uint32_t* d_sep_tpos;  /* [n_matches] */
} lra_seed_result;
int lra_seed_batch(lra_ctx* ctx, int n_reads, const char* d_seq, const uint64_t* d_read_off, int k, int w,
                   int max_freq, lra_seed_result* out);
/* A caller's match list as the context's current seed result, in the place of lra_seed_batch's: the input of lra_clean_matches_batch (which reads the matches and
 * nothing else of the seed stage), for tests that craft the matches.  Device arrays, CSR by read, every read's forward-strand matches first (the layout
 * SeparateMatchesByStrand leaves): d_match_off u64[n_reads + 1] (from 0, not decreasing), d_n_forward u32[n_reads] (<= the read's matches), d_qpos / d_tpos u32[m]
 * and d_qkey u64[m] (the read minimizer's key, AVGfreq's input), m = d_match_off[n_reads] < 2^32.  Copied device to device on the context's stream into the seed
 * stage's own arrays (grown as lra_seed_batch grows them); needs neither genome nor index.  `out` (may be NULL): the result as lra_seed_batch reports it, with no
 * minimizers and zeroed d_match_qi / d_match_ti.  LRA_ERR_INVALID for a malformed CSR.                                                                          */
int lra_seed_set_matches(lra_ctx* ctx, int n_reads, const uint64_t* d_match_off, const uint32_t* d_n_forward, const uint32_t* d_qpos, const uint32_t* d_tpos,
                         const uint64_t* d_qkey, lra_seed_result* out);

/* The seeding of the NEXT batch beside the current one.  The per-read path is a chain of launches that are as long as their largest reads: much of a batch's time the
 * device has room, and a1-a4 of the batch after it fit there.  `side` is a second context of the same device that shares the mapping context's reference data
 * (lra_ctx_share_reference), driven by a host thread of its own on its own (low-priority) stream: lra_seed_prefetch is lra_seed_batch on it, synchronous, the result
 * kept by `side`.  lra_ctx_adopt_seed(ctx, side) then hands that result to the mapping context (the two contexts exchange their seed-stage batch buffers; no copy);
 * the next lra_map_reads_lowacc_batch / lra_map_reads_highacc_batch on `ctx` with the same n_reads, d_seq, d_read_off and the same globalK / globalMaxFreq and the
 * w the batch sketches with (opts.globalW, or 1 on a context with lra_ctx_set_store_all on: prefetch with that w) starts from it instead of seeding -- with any other arguments it seeds as usual and the adopted result is dropped.  Same alignments either way: scheduling only.
 * The reads (d_seq, d_read_off) must stay untouched from the prefetch to the batch call.  Not combined with opts.defer_seed_matches (LRA_ERR_INVALID).
 * Replaces nothing in the reference: lra's worker threads (lra.cpp:678-714) each run MapRead start to end; this is the device's way of having two reads in flight. */
int lra_seed_prefetch(lra_ctx* side, int n_reads, const char* d_seq, const uint64_t* d_read_off, int k, int w, int max_freq);
int lra_ctx_adopt_seed(lra_ctx* ctx, lra_ctx* side);

/* CreateRC (SeqUtils.h:151): reverse complement of every read of the batch into d_rc (same offsets);
 * bytes other than ACGTacgtn become 'N' (RevCompNuc, SeqUtils.h:112).  Asynchronous.            */
int lra_create_rc_batch(lra_ctx* ctx, int n_reads, const char* d_seq, const uint64_t* d_read_off, char* d_rc);

/* a2 alone: sorts each list [d_off[i], d_off[i+1]) of (key,pos) tuples IN PLACE exactly as
 * `std::sort(readmm.begin(), readmm.end())` (MapRead.h:185, libstdc++ introsort with
 * GenomeTuple::operator<, TupleOps.h:76) would, including the order it leaves equal keys in.
 * Asynchronous.                                                                               */
int lra_sort_minimizers_batch(lra_ctx* ctx, int n_lists, const uint64_t* d_off, uint64_t* d_key, uint32_t* d_pos);
/* The same sort of ONE list of n (key,pos) tuples in HOST memory, in place, on the calling thread (additive to ABI 9; no context, no device): the host
 * instantiation of the library's restatement of std::sort, whose device instantiation takes the lists beyond 2^26 tuples.  Synchronous.             */
int lra_sort_minimizers_host(uint64_t n, uint64_t* h_key, uint32_t* h_pos);

/* The path's other sorts -- DiagonalSort / AntiDiagonalSort / CartesianSort of a read's (a cluster's, a gap's) matches (Sorting.h:50-150; called from
 * Clustering.h:1840 CleanMatches, ChainRefine.h:767 MergeChain's LinearExtend, LocalRefineAlignment.h:364), the sparse DP's point orders where no two
 * points of a list share a key (SparseDP.h:2171-2174), its diagonal order -- as one primitive: every segment [d_begin[i], d_end[i]) of (64-bit key,
 * 32-bit value) pairs sorted by the key bits [begin_bit, end_bit), STABLY (pairs with equal bits keep their input order: with the packed keys the
 * callers build, that is what std::sort leaves wherever the reference's comparator has no ties, and the callers send the lists with ties through
 * lra_sort_minimizers_batch), from (d_key_in, d_val_in) into (d_key_out, d_val_out); segments may be empty, need not be adjacent and must not overlap.
 * A segment of 257 .. 8192 pairs is sorted by one workgroup in LDS, the others by rocprim's segmented radix sort.  Asynchronous (the context's
 * stream); the work buffer is the context's.                                                                                                 */
int lra_sort_pairs_batch(lra_ctx* ctx, uint64_t n_pairs, uint64_t n_segments, const uint64_t* d_begin, const uint64_t* d_end, const uint64_t* d_key_in,
                         uint64_t* d_key_out, const uint32_t* d_val_in, uint32_t* d_val_out, int begin_bit, int end_bit);

/* ---- a5: match cleaning + diagonal clusters ----------------------------------------------
 * Replaces, per read and strand,   CleanMatches(Matches, clusters, genome, read, opts, timing, ma_strand)
 * (Clustering.h:1840) in the configuration every preset uses (opts.ExtractDiagonalFromClean, lra.cpp:268-431):
 * DiagonalSort / AntiDiagonalSort (Sorting.h:50,113) -> CleanOffDiagonal (Clustering.h:566-798, incl.
 * AVGfreq :550 and SecondRoundCleanOffDiagonal :802-868) -> one Cluster per surviving diagonal run
 * (SetClusterBoundariesFromMatches :308, chromIndex = header.Find(tStart) Genome.h:20).
 * Input: the forMatches / revMatches of lra_seed_batch (the context's current seed result).
 * Output (device arrays owned by the context, CSR by read; forward-strand clusters first, as
 * MapRead_lowacc builds `clusters`, Map_lowacc.h:77-78):
 *   clusters: per cluster start/end into the cleaned match arrays, q/t box, strand, chromIndex, anchorfreq
 *   cl_qpos / cl_tpos: the cleaned, diagonal-sorted matches (genome coordinates)                */
typedef struct lra_clean_opts {
  int32_t globalK, cleanMaxDiag, minDiagCluster, bypassClustering, cleanClustersize;
  int32_t SecondCleanMinDiagCluster, SecondCleanMaxDiag, punish_anchorfreq, anchorPerlength;
} lra_clean_opts;
typedef struct lra_cluster_result {
  int32_t n_reads;
  uint64_t n_clusters, n_matches;
  const uint64_t* d_cluster_off;  /* [n_reads+1] */
  const uint64_t* d_c_start;      /* [n_clusters] first match of the cluster (index into d_cl_*) */
  const uint64_t* d_c_end;        /* [n_clusters] one past its last match */
  const uint32_t* d_c_qStart; const uint32_t* d_c_qEnd; const uint32_t* d_c_tStart; const uint32_t* d_c_tEnd;
  const int32_t* d_c_strand; const int32_t* d_c_chrom; const float* d_c_anchorfreq;
  const uint32_t* d_cl_qpos; const uint32_t* d_cl_tpos;   /* [n_matches] */
} lra_cluster_result;
int lra_clean_matches_batch(lra_ctx* ctx, const lra_clean_opts* opts, const uint64_t* h_chrom_pos, int n_chrom,
                            lra_cluster_result* out);
/* The anchor bonus of the first sparse DP per read (Map_lowacc.h:86-89, :184-185): 3 for a read that has a cluster with anchorfreq in
 * (1, 2] and at least 500 matches ("repetitivecluster"), opts.initial_anchorbonus otherwise.  *d_rate: [n_reads] floats, context-owned;
 * pass it as d_rate to lra_sparse_dp_batch.  Asynchronous on the context's stream.                                                    */
int lra_match_rate_batch(lra_ctx* ctx, const lra_cluster_result* clusters, float initial_anchorbonus, const float** d_rate);

/* ---- a5 (high-accuracy path): MatchesToFineClusters -----------------------------------------------------------------------------------
 * Replaces   MatchesToFineClusters(forMatches, clusters, ...); MatchesToFineClusters(revMatches, clusters, ..., 1)   (Clustering.h:1555-1680,
 *            Map_highacc.h:41-42)
 * behind lra_clean_matches_batch run with the high-accuracy options (bypassClustering = 0: its clusters are the rough clusters of
 * CleanOffDiagonal): CartesianSort of every rough cluster, SplitRoughClustersWithGaps (:1358-1432), StoreFineClusters (:892-1331) for both
 * strands of every read, sharing the read's `clusters` vector as the reference does.  opts: Options::globalK, RoughClustermaxGap, maxDiag,
 * maxGap, minClusterSize, minUniqueStretchNum, minUniqueStretchDist (presets lra.cpp:268-340).
 * Output (context-owned): fine clusters CSR by read (d_cluster_off), their matches CSR by cluster (d_match_off over d_q / d_t, genome
 * coordinates), box {qStart, qEnd, tStart, tEnd}, strand, chromIndex, anchorfreq; d_status[r] = LRA_ST_OOB_SLOT where the reference reads
 * clusters.back() of an empty vector (:1305; the read then has no clusters).  Synchronous.                                               */
typedef struct lra_fine_opts { int32_t globalK, RoughClustermaxGap, maxDiag, maxGap, minClusterSize, minUniqueStretchNum, minUniqueStretchDist; } lra_fine_opts;
typedef struct lra_fine_result {
  int32_t n_reads;
  uint64_t n_clusters, n_matches;
  const uint64_t* d_cluster_off;   /* [n_reads+1] */
  const uint64_t* d_match_off;     /* [n_clusters+1] */
  const uint32_t* d_q; const uint32_t* d_t;   /* [n_matches] */
  const uint32_t* d_box;           /* [4*n_clusters] */
  const int32_t* d_strand; const int32_t* d_chrom; const float* d_anchorfreq;   /* [n_clusters] */
  const uint32_t* d_status;        /* [n_reads] */
} lra_fine_result;
int lra_fine_clusters_batch(lra_ctx* ctx, const lra_cluster_result* rough, const lra_fine_opts* opts, const uint64_t* h_chrom_pos, int n_chrom,
                            lra_fine_result* out);

/* ---- a7: linear extension of the cleaned clusters ------------------------------------------
 * Replaces, per cluster of the context's current lra_clean_matches_batch result,
 *   LinearExtend(&clusters[d].matches, ext.matches, ext.matchesLengths, opts, genome, read,
 *                chromIndex, strand, 1, opts.globalK)            (LinearExtend.h:658-716, Checkbp :50-85)
 *   DecideCoordinates(ext, strand, chromIndex, anchorfreq)        (LinearExtend.h:105-128)
 * as MapRead_lowacc does (Map_lowacc.h:131-137; chromosome offsets handled inside).  d_seq/d_read_off:
 * the reads of the batch (as given to lra_seed_batch).  Output: per cluster its extended anchors
 * (read pos, genome pos, length) at [d_e_start[c], d_e_start[c] + d_e_count[c]) and its new box.    */
typedef struct lra_extend_result {
  uint64_t n_clusters, n_anchors_cap;
  const uint64_t* d_e_start;      /* [n_clusters] */
  const uint32_t* d_e_count;      /* [n_clusters] */
  const uint32_t* d_e_qpos; const uint32_t* d_e_tpos; const int32_t* d_e_len;   /* [n_anchors_cap] */
  const uint32_t* d_box;          /* [4*n_clusters] qStart,qEnd,tStart,tEnd */
} lra_extend_result;
int lra_linear_extend_batch(lra_ctx* ctx, int K, const char* d_seq, const uint64_t* d_read_off, lra_extend_result* out);

/* ---- a7 (high-accuracy path): the cluster version of LinearExtend ---------------------------------------------------------------------
 * Replaces   LinearExtend_chain(chain, ExtendClusters, RefinedClusters, smallOpts, genome, read, start, overlap, skiprepetitive, K)
 *            (LinearExtend.h:783-792) = LinearExtend(vector<Cluster*>, vector<Cluster>&, chain, ...) (:136-352; CheckOverlap :88, Checkbp :50,
 *            DecideCoordinates :105) + TrimOverlappedAnchors(ExtendClusters, start) (:574-649), called at Map_highacc.h:580 for every chain.
 * Item i = one element of one chain: the refined cluster d_item_cluster[i], its neighbours on the chain d_item_prev[i] / d_item_next[i]
 * (cluster indices, -1 at the ends), the read d_item_read[i].  Refined clusters: matches CSR d_match_off over d_mq / d_mt (t relative to the
 * cluster's chromosome; SORTED IN PLACE by diagonal / anti-diagonal as the reference does, :201-210), d_box {qStart, qEnd, tStart, tEnd} (t
 * relative), d_strand, d_chrom, d_anchorfreq.  d_seq / d_read_off: the reads (forward); d_genome: all chromosomes.
 * Output (context-owned): per item its anchors d_anchor_off[i] .. d_anchor_off[i+1] (read pos, chromosome pos, length, Cluster::overlap flag),
 * and what DecideCoordinates leaves: box, strand (-1 for an element without matches: the Cluster() default), chromIndex, anchorfreq.
 * trim != 0 applies TrimOverlappedAnchors to every item's list.  Synchronous.                                                              */
typedef struct lra_ext_clusters_result {
  uint64_t n_items, n_anchors;
  const uint64_t* d_anchor_off;    /* [n_items+1] */
  const uint32_t* d_q; const uint32_t* d_t; const int32_t* d_len; const uint8_t* d_overlap;   /* [n_anchors] */
  const uint32_t* d_box; const int32_t* d_strand; const int32_t* d_chrom; const float* d_anchorfreq;   /* [4*n_items], [n_items] */
} lra_ext_clusters_result;
int lra_linear_extend_clusters_batch(lra_ctx* ctx, uint64_t n_items, const uint32_t* d_item_cluster, const int32_t* d_item_prev, const int32_t* d_item_next,
                                     const uint32_t* d_item_read, uint64_t n_clusters, const uint64_t* d_match_off, uint64_t n_matches, uint32_t* d_mq, uint32_t* d_mt,
                                     const uint32_t* d_box, const int32_t* d_strand, const int32_t* d_chrom, const float* d_anchorfreq, const char* d_seq,
                                     const uint64_t* d_read_off, const char* d_genome, const uint64_t* h_chrom_pos, int n_chrom, int skiprepetitive, int K, int trim,
                                     lra_ext_clusters_result* out);

/* ---- a8: sparse dynamic programming over the extended anchors ("SDP#A") -------------------------
 * Replaces, per read,   SparseDP(ext_clusters, chains, optsSDP, LookUpTable, read, match_rate)
 * (SparseDP.h:2139-2279 as called from Map_lowacc.h:188): insertPointsPair (:79), the SortByRowOp / SortByColOp
 * std::sorts (:2171-2174, libstdc++ permutation of tied points included), GetRowInfo / GetColInfo, the four
 * decompositions DivideSubProbBy{Row,Col}{1,2}, ProcessPoint<Cluster> (:1015) with Maximization /
 * FindValueInBlock / PWL_w (SubRountine.h), PassValueToD1/D2 (:140,:226), the Fragment_valueOrder sort,
 * TraceBack (:1351) and DecidePrimaryChains (:1658).  InitPWL(gapopen, gapextend, gaproot, gapCeiling1,
 * gapCeiling2) (lra.cpp:648) is evaluated on the host with the host libm, as the reference does at start-up.
 * Input: clusters CSR by read (d_cluster_off[n_reads+1]); per cluster its anchors
 * [d_c_start[c], d_c_start[c] + d_c_count[c]) in d_q/d_t/d_len (read pos, GLOBAL genome pos, length -- the layout
 * lra_linear_extend_batch produces) and its strand; read lengths from d_read_off; match_rate per read
 * (d_rate, NULL = opts->rate for every read; Map_lowacc.h:185-186 uses 3 for reads with a repetitive cluster).
 * Output (context-owned, valid until the next call): per read up to opts->NumAln chains in slots
 * [r*NumAln, r*NumAln + d_n_chains[r]); slot s: anchors d_chain_cluster/anchor/link[d_chain_start[s] .. + d_chain_len[s])
 * in trace-back order (last anchor first; cluster = index within the read, anchor = index within the cluster,
 * link[i] = 1 if the step to the next listed anchor is an inversion link), box = QStart,QEnd,TStart,TEnd,
 * value = FirstSDPValue.  d_frag_off[n_reads+1] / d_frag_val: every anchor's final DP value in cluster order.
 * mode LRA_SDP_SINGLE_CLUSTER replaces  SparseDP(ClusterIndex, extend_clusters, ultimatechain, smallOpts, LookUpTable, read)
 * (SparseDP.h:2287-2438, called at Map_lowacc.h:535): every "read" is one cluster job, anchors get only their own family's point pair,
 * rate = opts.second_anchorbonus, and the one chain is the plain TraceBack (:1521) from the first anchor of maximal value (no box).
 * The same mode with several clusters per job is  SparseDP(SplitChain& inputChain, vector<Cluster_SameDiag*>&, FinalChain&, ...)
 * (SparseDP.h:1766-1955, LocalRefineAlignment.h:563): pass the clusters of inputChain in order, anchors = (GetqStart, GettStart, length).
 * SparseDP_ForwardOnly (SparseDP_Forward.h:312-450, called at LocalRefineAlignment.h:378) is this mode on one forward-strand cluster
 * per job with rate = (float)rate: the same points, weights, first-maximum rule and trace back.
 * d_status[r]: LRA_ST_CAPACITY if a work buffer bound was hit, LRA_ST_OOB_SLOT if the reference would read outside
 * its arrays (the read then has no chains).  Synchronous.                                              */
#define LRA_SDP_CLUSTERS 0
#define LRA_SDP_SINGLE_CLUSTER 1
typedef struct lra_sdp_opts {
  float rate; int32_t NumAln; float alnthres;
  float gapopen, gapextend, gaproot; int32_t gapCeiling1, gapCeiling2;
  int32_t mode;   /* LRA_SDP_CLUSTERS (0) or LRA_SDP_SINGLE_CLUSTER (1) */
  int32_t globalK; /* Options::globalK; read by lra_sparse_dp_boxes_batch only (value threshold, SparseDP.h:1592) */
} lra_sdp_opts;
typedef struct lra_chain_result {
  int32_t n_reads, num_aln;
  uint64_t n_frags, n_points, n_subproblem_entries;
  const uint32_t* d_n_chains;       /* [n_reads] */
  const uint64_t* d_chain_start;    /* [n_reads*num_aln] */
  const uint32_t* d_chain_len;      /* [n_reads*num_aln] */
  const uint32_t* d_chain_box;      /* [4*n_reads*num_aln] */
  const float* d_chain_value;       /* [n_reads*num_aln] */
  const uint32_t* d_chain_cluster; const uint32_t* d_chain_anchor; const uint8_t* d_chain_link;   /* [n_frags] */
  const uint32_t* d_chain_q; const uint32_t* d_chain_t; const int32_t* d_chain_alen; const uint8_t* d_chain_strand;   /* [n_frags] the anchors themselves (q, t, length, strand of the cluster) */
  const uint64_t* d_frag_off;       /* [n_reads+1] */
  const float* d_frag_val;          /* [n_frags] */
  const uint32_t* d_status;         /* [n_reads] */
  const int32_t* d_chain_num_anchors; /* [n_reads*num_aln] CHain::NumOfAnchors0 (lra_sparse_dp_boxes_batch; NULL otherwise) */
} lra_chain_result;
int lra_sparse_dp_batch(lra_ctx* ctx, int n_reads, const uint64_t* d_cluster_off, const uint64_t* d_c_start, const uint32_t* d_c_count,
                        const int32_t* d_c_strand, const uint32_t* d_q, const uint32_t* d_t, const int32_t* d_len,
                        const uint64_t* d_read_off, const float* d_rate, const lra_sdp_opts* opts, lra_chain_result* out);

/* The high-accuracy overload SparseDP(vector<Cluster>& splitclusters, vector<Primary_chain>&, opts, LookUpTable, read,
 * rate) (SparseDP.h:1956-2135, called at Map_highacc.h:229): every box contributes the four points s1 (qStart+1, tStart+1), e1 (qEnd-1,
 * tEnd-1), s2 (qStart+1, tEnd-1), e2 (qEnd-1, tStart+1) in that insertion order, weighs Val*rate (ProcessPoint :313), and chains are
 * chosen by DecidePrimaryChains :1587-1655: value threshold max(alnthres*best, best - 130*globalK), TraceBack with `used`, box by
 * min/max over the chain, read-span fraction > 0.005, at most NumAln chains (they are Primary_chains[0].chains).
 * Box i of read r is d_box_off[r] + i: (d_qs, d_qe, d_ts, d_te, d_strand 0 = forward, d_val = Cluster::Val, d_num_anchors =
 * Cluster::NumofAnchors0, may be NULL).  opts->rate (or d_rate[r]) is the caller's `rate` (Map_highacc.h:227-228); opts->mode is
 * ignored.  Result as lra_sparse_dp_batch: d_chain_cluster = box index within the read, d_chain_q/t = (qStart, tStart),
 * d_chain_alen = Val, d_chain_anchor = 0, plus d_chain_num_anchors (ComputeNumOfAnchors :1577).                         */
int lra_sparse_dp_boxes_batch(lra_ctx* ctx, int n_reads, const uint64_t* d_box_off, const uint32_t* d_qs, const uint32_t* d_qe,
                              const uint32_t* d_ts, const uint32_t* d_te, const int32_t* d_strand, const int32_t* d_val,
                              const int32_t* d_num_anchors, const uint64_t* d_read_off, const float* d_rate, const lra_sdp_opts* opts,
                              lra_chain_result* out);

/* ---- a6 (high-accuracy path): SplitClusters + DecideSplitClustersValue -----------------------------------
 * Replaces, for every read of a batch, SplitClusters(clusters, splitclusters, read, opts) (SplitClusters.h:63-171, IntervalSet :18-60)
 * and DecideSplitClustersValue(clusters, splitclusters, opts, read) (:176-249) as called at Map_highacc.h:153-155.
 * Cluster c of read r is d_cluster_off[r] + c: box (d_qs, d_qe, d_ts, d_te), d_strand (0 = forward), d_anchorfreq; its matches' read
 * positions (matches[i].first.pos, in the cluster's own CartesianSort order) are d_match_q[d_match_off[c] .. d_match_off[c+1]).
 * contig = (opts.readType == Options::contig) (only then are sparse clusters kept whole), K = opts.globalK.
 * Output (context-owned): split clusters of read r = [d_split_off[r], d_split_off[r+1]) of d_qs.. in the reference's push order (whole
 * clusters first, then pieces cluster by cluster): box, strand, d_coarse (index of the original within the read), d_val (Cluster::Val),
 * d_num_anchors (NumofAnchors0), d_read; per original cluster d_cluster_val (Cluster::Val) and d_cluster_split (Cluster::split).
 * The arrays feed lra_sparse_dp_boxes_batch unchanged.  Synchronous.                                                              */
typedef struct lra_split_clusters_result {
  int32_t n_reads; uint64_t n_clusters, n_split;
  const uint64_t* d_split_off;                 /* [n_reads+1] */
  const uint32_t* d_qs; const uint32_t* d_qe; const uint32_t* d_ts; const uint32_t* d_te;   /* [n_split] */
  const int32_t* d_strand; const int32_t* d_coarse; const int32_t* d_val; const int32_t* d_num_anchors; const uint32_t* d_read;   /* [n_split] */
  const int32_t* d_cluster_val; const uint8_t* d_cluster_split;   /* [n_clusters] */
} lra_split_clusters_result;
int lra_split_clusters_batch(lra_ctx* ctx, int n_reads, const uint64_t* d_cluster_off, const uint32_t* d_qs, const uint32_t* d_qe,
                             const uint32_t* d_ts, const uint32_t* d_te, const int32_t* d_strand, const float* d_anchorfreq,
                             const uint64_t* d_match_off, const uint32_t* d_match_q, int contig, int K, lra_split_clusters_result* out);

/* ---- a9 (low-accuracy path): chain filters and chain splitting -------------------------------------------
 * Replaces, per chain of an lra_sparse_dp_batch result (mode LRA_SDP_CLUSTERS), what MapRead_lowacc does before tier-2 refinement:
 *   RemoveSpuriousJump<UltimateChain>(chains[p])                                   Chain.h:897-957   (Map_lowacc.h:189-192)
 *   SPLITChain(genome, read, chains[p], spchain, spchain_link, opts)               Mapping_ultility.h:385-441 (push_new :349,
 *     SplitChain::CHROMIndex Chain.h:386, MergeSplitchainINS Mapping_ultility.h:172)
 *   RemoveSpuriousSplitChain(spchain, spchain_link)                                Map_lowacc.h:38-66
 * h_chrom_pos = genome.header.pos (n_chrom + 1 entries).  Output (context-owned), all arrays indexed like the chain arrays: chain
 * slot s occupies [d_chain_start[s], + d_chain_len[s]):
 *   d_keep[i]            1 if anchor i of the chain survives RemoveSpuriousJump; d_n_kept[s]; d_link[.. + n_kept-1) the filtered links
 *   d_n_split[s]         number of split chains; split k of slot s lives at index x = d_chain_start[s] + k of the per-split arrays:
 *   d_sp_beg[x], d_sp_len[x]   its anchors = d_sp_idx[d_chain_start[s] + beg .. + len) (indices into the FILTERED chain, in the
 *                        order SPLITChain leaves them: forward-strand pieces reversed), d_sp_link alongside (len-1 used)
 *   d_sp_type[x] ('N','T','I'), d_sp_strand[x], d_sp_chrom[x], d_sp_box[4x..] (QStart,QEnd,TStart,TEnd)
 *   d_ci_beg[x], d_ci_len[x]   SplitChain::ClusterIndex = d_ci_idx[d_chain_start[s] + beg .. + len)
 *   d_split_link[d_chain_start[s] + k], k < d_n_split_link[s]     spchain_link
 *   d_status[s]          LRA_ST_OOB_SLOT if the reference would read outside its arrays (the slot then has no splits).  Synchronous. */
typedef struct lra_split_result {
  uint64_t n_slots, n_frags;
  const uint8_t* d_keep; const uint32_t* d_n_kept; const uint8_t* d_link;
  const uint32_t* d_n_split; const uint32_t* d_sp_beg; const uint32_t* d_sp_len; const uint32_t* d_sp_idx; const uint8_t* d_sp_link;
  const uint8_t* d_sp_type; const uint8_t* d_sp_strand; const int32_t* d_sp_chrom; const uint32_t* d_sp_box;
  const uint32_t* d_ci_beg; const uint32_t* d_ci_len; const uint32_t* d_ci_idx;
  const uint8_t* d_split_link; const uint32_t* d_n_split_link; const uint32_t* d_status;
  const uint32_t* d_fidx;   /* [n_frags] position in the filtered chain -> position in the chain (both relative to d_chain_start[s]) */
} lra_split_result;
int lra_split_chains_batch(lra_ctx* ctx, const lra_chain_result* chains, const uint64_t* h_chrom_pos, int n_chrom, int splitdist,
                           int bypass_clustering, lra_split_result* out);

/* The chain filters of Chain.h on arbitrary chains (CSR d_off[n_chains+1] over anchors given by read pos, genome pos, length, strand of the
 * cluster, trace-back order; d_link[i] = link bit between anchor i and i+1 of the same chain, NULL if the chain type has none), applied in
 * the order h_ops[0..n_ops):  1 RemoveSmallPairedIndels (:546)   2 RemovePairedIndels (:607)   3 the same with refineEnds = false
 *   5 RemovePairedIndels(GenomePairs&, chain, lengths) (:753-811; strand and link are not read)
 * 4 RemoveSpuriousAnchors (:828; leaves `link` longer than the chain, as the reference does)   8 RemoveSpuriousJump (:897).
 * Map_lowacc.h:538-539 = {2, 4};  LocalRefineAlignment.h:567-571 = {1, 2 (or 3), 4}.
 * Output (context-owned; shares its buffer with lra_split_chains_batch): d_keep per anchor, d_n_kept per chain, the surviving links
 * d_link[d_off[c] .. + d_n_link[c]).  Synchronous.                                                                               */
typedef struct lra_filter_result {
  uint64_t n_chains, n_anchors;
  const uint8_t* d_keep; const uint32_t* d_n_kept; const uint8_t* d_link; const uint32_t* d_n_link;
} lra_filter_result;
int lra_filter_chains_batch(lra_ctx* ctx, uint64_t n_chains, const uint64_t* d_off, uint64_t n_anchors, const uint32_t* d_q, const uint32_t* d_t,
                            const int32_t* d_len, const uint8_t* d_strand, const uint8_t* d_link, const int32_t* h_ops, int n_ops,
                            lra_filter_result* out);
/* The same with the chain's qEnd(i) given explicitly (d_qend[i]; NULL = q + length): FinalChain::qEnd is Cluster_SameDiag::GetqEnd
 * (Clustering.h:378-380), the merged entry's length added to its LAST anchor's read position; the high-accuracy LocalRefineAlignment
 * (LocalRefineAlignment.h:567-571) filters such chains.                                                                              */
int lra_filter_chains_ex_batch(lra_ctx* ctx, uint64_t n_chains, const uint64_t* d_off, uint64_t n_anchors, const uint32_t* d_q, const uint32_t* d_t,
                               const int32_t* d_len, const uint32_t* d_qend, const uint8_t* d_strand, const uint8_t* d_link, const int32_t* h_ops, int n_ops,
                               lra_filter_result* out);

/* ---- a10: tier-2 (local) minimizer index and lookups ----------------------------------------
 * lra_local_index_batch replaces  LocalIndex::IndexSeq(char* seq, int seqLen)  (MMIndex.h:200-245) for
 * n_seqs sequences (read strands, Map_lowacc.h:246-250; or chromosomes = LocalIndex::IndexFile, the
 * `.gli` payload): per `window` bases the non-canonical (w,k) minimizers (MinCount.h:182), sorted by
 * k-mer with std::sort (MMIndex.h:219) and thinned by RemoveFrequent(maxFreq) (MMIndex.h:69).
 * LocalTuple = uint32  t | pos << 20  (TupleOps.h:20-25; pos relative to the window start).
 * Result (one context-owned allocation of `bytes` bytes starting at d_base, valid until the next call;
 * copy it with lra_copy_device to keep several indexes alive): d_win_off[n_seqs+1] (first window of
 * each sequence), d_tuple_bnd[n_windows+1] (tupleBoundaries), d_tuples[n_tuples].  Synchronous.
 *
 * lra_local_compare_batch replaces  CompareLists<LocalTuple,SmallTuple>(qBegin,qEnd,tBegin,tEnd,result,
 * opts,false,maxDiagNum,minDiagNum)  (CompareLists.h:9) for n_tasks (query list, target list) pairs
 * given as index ranges into two tuple arrays; max_freq = opts.localMaxFreq; per-task diagonal bounds
 * (NULL = unbounded; the filter applies only when both are non-zero, CompareLists.h:87).  Output: the
 * emitted pairs as absolute indices into the two tuple arrays, CSR by task, in the reference's order
 * (context-owned, valid until the next call).  Synchronous.  Both tuple arrays must be 16-byte aligned
 * and readable up to the next 32-byte boundary beyond their last tuple (the walk of large tasks fetches
 * whole 8-word lines); the d_tuples of the library's own index results satisfy this.               */
typedef struct lra_local_index_result {
  int32_t n_seqs;
  uint64_t n_windows, n_tuples, bytes;
  const void* d_base;
  const uint64_t* d_win_off; const uint64_t* d_tuple_bnd; const uint32_t* d_tuples;
} lra_local_index_result;
int lra_local_index_batch(lra_ctx* ctx, int n_seqs, const char* d_seq, const uint64_t* d_seq_off, int k, int w, int window,
                          int max_freq, lra_local_index_result* out);
/* The same with sequences switched off: d_active[s] == 0 leaves sequence s's windows in place (the window numbering is unchanged) but empty.
 * MapRead_lowacc indexes both strands of every read (Map_lowacc.h:249-250) and then only looks up the strands its split chains lie on.       */
int lra_local_index_masked_batch(lra_ctx* ctx, int n_seqs, const char* d_seq, const uint64_t* d_seq_off, const uint8_t* d_active, int k, int w,
                                 int window, int max_freq, lra_local_index_result* out);
typedef struct lra_local_pairs_result {
  uint64_t n_tasks, n_pairs;
  const uint64_t* d_pair_off; const uint32_t* d_pair_qi; const uint32_t* d_pair_ti;
} lra_local_pairs_result;
int lra_local_compare_batch(lra_ctx* ctx, uint64_t n_tasks, const uint32_t* d_q_tuples, const uint64_t* d_q_lo, const uint64_t* d_q_hi,
                            const uint32_t* d_t_tuples, const uint64_t* d_t_lo, const uint64_t* d_t_hi, int max_freq,
                            const int64_t* d_max_diag, const int64_t* d_min_diag, lra_local_pairs_result* out);

/* Refine_splitchain(splitchains, chain, refinedclusters, clusters, genome, read, glIndex, localIndexes, smallOpts, opts)
 * (ChainRefine.h:384-576, called at Map_lowacc.h:294) for every split chain of an lra_split_chains_batch result: the walk over the
 * genome local-index windows under the split chain (LocalIndex::LookupIndex MMIndex.h:175, GenomeHeader::GetNextOffset Genome.h:43),
 * with the extended clusters of the split chain brought to chromosome coordinates on their own strand (SwapStrand ClusterRefine.h:24,
 * K = opts.globalK), CompareLists<LocalTuple,SmallTuple> of every (read window, genome window) it meets, AppendValues
 * (TupleOps.h:159-195), SwapStrand of reverse results (K = smallOpts.globalK), SetClusterBoundariesFromMatches (Clustering.h:308) and
 * refineEffiency.
 * read_index: ONE lra_local_index_batch result over 2*n_reads sequences, the reads forward then their reverse complements
 * (forwardIndex / reverseIndex, Map_lowacc.h:246-250), built with window = opts->local_window.  Genome local index (`.gli` payload):
 * d_g_seq_off[n_g_windows+1] = glIndex.seqOffsets, d_g_tuple_bnd = tupleBoundaries, d_g_tuples = minimizers.
 * opts: window = smallOpts.window, smallK = smallOpts.globalK, K = opts.globalK, limitrefine = opts.limitrefine, max_freq =
 * smallOpts.localMaxFreq, local_window = glIndex.localIndexWindow.
 * UNDEFINED IN THE REFERENCE: with limitrefine (the default) the upper diagonal bound of every window starts from an uninitialised
 * variable (ChainRefine.h:468 `miniMaxDiag = miniMaxDiag;`); here it starts from the first anchor's diagonal like the lower bound.
 * Output (context-owned), indexed like the split arrays (split k of slot s at x = d_chain_start[s] + k): refinedclusters[k].matches =
 * (d_match_q, d_match_t)[d_match_off[x] .. d_match_off[x+1]) (t relative to the chromosome), d_box[4x..] = qStart,qEnd,tStart,tEnd,
 * d_eff[x] = refineEffiency, d_status[x] (LRA_ST_OOB_SLOT where the reference would index outside an array; no matches then).
 * strand / coarse / chromIndex of the refined cluster are the split chain's Strand / k / chromIndex.  Synchronous.            */
typedef struct lra_rsc_opts { int32_t window, smallK, K, limitrefine, max_freq, local_window; } lra_rsc_opts;
typedef struct lra_refined_result {
  uint64_t n_frags, n_tasks, n_pairs, n_matches;
  const uint64_t* d_match_off;               /* [n_frags+1] */
  const uint32_t* d_match_q; const uint32_t* d_match_t;   /* [n_matches] */
  const uint32_t* d_box; const float* d_eff; const uint32_t* d_status;   /* [4*n_frags], [n_frags], [n_frags] */
  const uint64_t* d_task_q_lo; const uint64_t* d_task_q_hi; const uint64_t* d_task_t_lo; const uint64_t* d_task_t_hi;   /* [n_tasks] the CompareLists calls, as tuple ranges */
} lra_refined_result;
int lra_refine_splitchain_batch(lra_ctx* ctx, const lra_chain_result* chains, const lra_split_result* split, const uint64_t* d_read_off,
                                const uint64_t* h_chrom_pos, int n_chrom, const lra_local_index_result* read_index, uint64_t n_g_windows,
                                const uint64_t* d_g_seq_off, const uint64_t* d_g_tuple_bnd, const uint32_t* d_g_tuples,
                                const lra_rsc_opts* opts, lra_refined_result* out);

/* REFINEclusters(clusters, refinedclusters, genome, read, glIndex, localIndexes, smallOpts, opts) (ClusterRefine.h:50-240, called at
 * Map_highacc.h:429-447): the cluster-wise twin of Refine_splitchain on the high-accuracy path.  Cluster c of read r is d_cluster_off[r] + c:
 * its matches are (d_q, d_t genome-wide)[d_c_start[c] .. + d_c_count[c]) (n_matches_cap = the extent of those arrays), its box d_qs/d_qe/
 * d_ts/d_te (genome-wide t), d_c_strand.  read_index / genome index / opts as for lra_refine_splitchain_batch (limitrefine unused).
 * Output (context-owned, shares buffers with lra_refine_splitchain_batch): per cluster d_chrom (Cluster::CHROMIndex), d_status
 * (LRA_ST_REJECTED: the cluster spans two chromosomes and is cleared, :61-65; LRA_ST_OOB_SLOT), refined matches CSR (t relative to the
 * chromosome), box, refineEffiency.  strand / coarse (-1) / refinespace (0) are the caller's.  Synchronous.                          */
typedef struct lra_refined_clusters_result {
  uint64_t n_clusters, n_tasks, n_pairs, n_matches;
  const uint64_t* d_match_off; const uint32_t* d_match_q; const uint32_t* d_match_t;
  const uint32_t* d_box; const float* d_eff; const uint32_t* d_status; const int32_t* d_chrom;
} lra_refined_clusters_result;
int lra_refine_clusters_batch(lra_ctx* ctx, int n_reads, const uint64_t* d_cluster_off, const uint64_t* d_c_start, const uint32_t* d_c_count,
                              const int32_t* d_c_strand, const uint32_t* d_qs, const uint32_t* d_qe, const uint32_t* d_ts, const uint32_t* d_te,
                              const uint32_t* d_q, const uint32_t* d_t, uint64_t n_matches_cap, const uint64_t* d_read_off, const uint64_t* h_chrom_pos,
                              int n_chrom, const lra_local_index_result* read_index, uint64_t n_g_windows, const uint64_t* d_g_seq_off,
                              const uint64_t* d_g_tuple_bnd, const uint32_t* d_g_tuples, const lra_rsc_opts* opts, lra_refined_clusters_result* out);

/* ---- a11: anchors inside one gap ------------------------------------------------------------------------
 * Replaces   float RefineSpace(int K, int W, int refineSpaceDiag, bool consider_str, GenomePairs& EndPairs, const Options& opts,
 *                              Genome&, Read&, char* strands[2], int& ChromIndex, GenomePos qe, GenomePos qs, GenomePos te, GenomePos ts,
 *                              bool st, GenomePos lrts = 0, GenomePos lrlength = 0)                     (ClusterRefine.h:242-325)
 * for n gaps.  Gap p: query = d_qseq[q_off .. + q_len) (= strands[st] + qs, q_len = qe - qs), target = d_tseq[t_off .. + t_len)
 * (= genome.seqs[ChromIndex] + (ts - lrts), t_len = te - ts + lrlength), t_span = te - (ts - lrts) (GenomePos arithmetic, used for the
 * diagonal band), K / W / diag = refineSpaceDiag per gap, q_add = qs, t_add = ts - lrts, flip_len = read.length if (consider_str and
 * st == 1) else 0.  match / mismatch / indel = opts.localMatch / localMismatch / localIndel, max_freq = opts.localMaxFreq of the
 * Options the caller passes (CompareLists with Global = false).  Output (context-owned): EndPairs as (first.pos, second.pos) CSR by gap,
 * in the reference's order; identity (the return value: matching bases / min(span) when both spans are < 1000, else -1); status (the
 * AffineOneGapAlign status bits, LRA_ST_RANGE for W > 32).  Synchronous.                                                      */
typedef struct lra_refine_space_result {
  uint64_t n_problems, n_pairs, n_small;
  const uint64_t* d_pair_off; const uint32_t* d_pair_q; const uint32_t* d_pair_t; const float* d_identity; const uint32_t* d_status;
} lra_refine_space_result;
int lra_refine_space_batch(lra_ctx* ctx, int n, const char* d_qseq, const uint64_t* d_q_off, const int32_t* d_q_len, const char* d_tseq,
                           const uint64_t* d_t_off, const int32_t* d_t_len, const uint32_t* d_t_span, const int32_t* d_K, const int32_t* d_W,
                           const int32_t* d_diag, const uint32_t* d_q_add, const uint32_t* d_t_add, const uint32_t* d_flip_len, int match,
                           int mismatch, int indel, int max_freq, lra_refine_space_result* out);
/* the same with opts.localMaxFreq given per gap (d_max_freq[n]) */
int lra_refine_space_batch_mf(lra_ctx* ctx, int n, const char* d_qseq, const uint64_t* d_q_off, const int32_t* d_q_len, const char* d_tseq,
                              const uint64_t* d_t_off, const int32_t* d_t_len, const uint32_t* d_t_span, const int32_t* d_K, const int32_t* d_W,
                              const int32_t* d_diag, const uint32_t* d_q_add, const uint32_t* d_t_add, const uint32_t* d_flip_len, int match,
                              int mismatch, int indel, const int32_t* d_max_freq, lra_refine_space_result* out);

/* Refine_Btwnsplitchain(spchain, refined_clusters, RevBtwnCluster, tracerev, genome, read, smallOpts, strands, spchain_link)
 * (ChainRefine.h:579-754, called at Map_lowacc.h:362) for every chain of the batch: for each pair of neighbouring refined clusters the
 * case analysis of :587-660 (plain gap, INV, DUP) and RefineBtwnSpace_AppendCloseCluster (:59-121; append_to_closetcluster :22-56) /
 * RefineBtwnSpace (ClusterRefine.h:327-430) on the one or two spaces, then the spaces beyond the first and the last split chain
 * (:684-753), each RefineSpace call going through lra_refine_space_batch.  Gaps of one chain are taken in order (a gap reads the boxes
 * the previous one may have moved): the batch advances in rounds, one gap index per round.
 * refined = the lra_refine_splitchain_batch result of the same chains / split; d_strands = the reads forward, then (at byte rc_base)
 * their reverse complements, laid out by d_read_off; d_genome = all chromosomes back to back (h_chrom_pos).  opts = the Options the
 * reference passes (smallOpts): K / W = globalK / globalW, refineSpaceDist, anchorstoosparse, localMatch / localMismatch / localIndel,
 * max_freq = localMaxFreq.  Read types -ONT / -CLR only (the others leave refineSpaceDiag uninitialised, ChainRefine.h:68-71).
 * Output (context-owned), indexed like the split arrays: the refined clusters after the call -- matches (base matches first, then every
 * appended run in the reference's order), box, refineEffiency, refinespace flag.  RevBtwnCluster / tracerev are dead in the reference
 * (their consumer is commented out, Map_lowacc.h:363-370) and are not produced.  Synchronous.                                    */
typedef struct lra_btwn_opts { int32_t K, W, refineSpaceDist; float anchorstoosparse; int32_t match, mismatch, indel, max_freq; } lra_btwn_opts;
typedef struct lra_btwn_result {
  uint64_t n_frags, n_matches, n_problems, n_pairs; uint32_t n_rounds;
  const uint64_t* d_match_off; const uint32_t* d_match_q; const uint32_t* d_match_t;
  const uint32_t* d_box; const float* d_eff; const uint8_t* d_refinespace;
} lra_btwn_result;
int lra_refine_btwn_splitchain_batch(lra_ctx* ctx, const lra_chain_result* chains, const lra_split_result* split, const lra_refined_result* refined,
                                     const uint64_t* d_read_off, const char* d_strands, uint64_t rc_base, const char* d_genome,
                                     const uint64_t* h_chrom_pos, int n_chrom, const lra_btwn_opts* opts, lra_btwn_result* out);

/* What MapRead_lowacc does with the refined clusters of every chain before the second sparse DP (Map_lowacc.h:440-476):
 *   MergeChain(Refined_Clusters, mergeinfo, merge_spcluster, spcluster)                         ChainRefine.h:767-802
 *   LinearExtend(&Refined_Clusters[cI]->matches, extend_clusters[r].matches, .matchesLengths, smallOpts, genome, read, chromIndex,
 *                st, 0, smallOpts.globalK) for every member of a merged cluster                     LinearExtend.h:658-716
 *   DecideCoordinates(extend_clusters[r], st, chromIndex, anchorfreq)                             LinearExtend.h:105-127
 *   TrimOverlappedAnchors(extend_clusters, 0)                                                     LinearExtend.h:574-649
 * refined = the lra_refine_btwn_splitchain_batch result; d_seq = the reads (forward), d_genome = all chromosomes; K = smallOpts.globalK.
 * Output (context-owned): merged cluster g of chain slot s is d_slot_group_off[s] + g; it covers the refined clusters (dense index
 * d_cluster_base[s] + k for split chain k) d_group_first[g] .. d_group_last[g]; its anchors are (d_q, d_t chromosome-relative, d_len)
 * [d_anchor_off[g], + d_count[g]); d_box[4g..] / d_strand / d_chrom as DecideCoordinates leaves them.
 * The second sparse DP (Map_lowacc.h:535) is lra_sparse_dp_batch in mode LRA_SDP_SINGLE_CLUSTER with n_reads = n_groups,
 * d_cluster_off = d_iota, d_c_start = d_anchor_off, d_c_count = d_count, d_c_strand = d_strand, d_q / d_t / d_len.  Synchronous.   */
typedef struct lra_merge_result {
  uint64_t n_slots, n_groups, n_anchors;
  const uint64_t* d_slot_group_off;   /* [n_slots+1] */
  const uint64_t* d_cluster_base;     /* [n_slots+1] */
  const uint32_t* d_group_slot; const uint32_t* d_group_first; const uint32_t* d_group_last;   /* [n_groups] */
  const uint64_t* d_anchor_off;       /* [n_groups+1] */
  const uint32_t* d_count;            /* [n_groups] */
  const uint32_t* d_q; const uint32_t* d_t; const int32_t* d_len;   /* [n_anchors] */
  const uint32_t* d_box; const int32_t* d_strand; const int32_t* d_chrom;   /* [4*n_groups], [n_groups] */
  const uint64_t* d_iota;             /* [n_groups+1] 0, 1, 2, ... */
} lra_merge_result;
/* TrimOverlappedAnchors(GenomePairs&, vector<int>&) (LinearExtend.h:722-780; used at LocalRefineAlignment.h:371): n_lists anchor lists in CSR
 * d_off, lengths trimmed in place.  Synchronous.                                                                                          */
int lra_trim_anchor_pairs_batch(lra_ctx* ctx, uint64_t n_lists, const uint64_t* d_off, uint64_t n_anchors, uint32_t* d_q, uint32_t* d_t, int32_t* d_len);
/* TrimOverlappedAnchors(vector<Cluster>& extCluster, int start) (LinearExtend.h:574-649; LinearExtend_chain :783, Map_lowacc.h:476): the cluster
 * version -- long anchors are those of 40 bases or more, a reverse-strand cluster (d_strand[c] == 1) is walked by read end and has the
 * read start of the trimmed anchor moved; read positions and lengths are changed in place.  Synchronous.                                    */
int lra_trim_overlapped_anchors_batch(lra_ctx* ctx, uint64_t n_clusters, const uint64_t* d_off, uint64_t n_anchors, const int32_t* d_strand,
                                      uint32_t* d_q, uint32_t* d_t, int32_t* d_len);
int lra_merge_extend_batch(lra_ctx* ctx, const lra_chain_result* chains, const lra_split_result* split, const lra_btwn_result* refined, const char* d_seq,
                           const uint64_t* d_read_off, const char* d_genome, const uint64_t* h_chrom_pos, int n_chrom, int K, lra_merge_result* out);

/* ---- a12: banded one-gap seed-extension DP ------------------------------------------
 * Replaces   int AffineOneGapAlign(string& qSeq, int qLen, string& tSeq, int tLen,
 *                                  int m, int mm, int indel, int k, Alignment& aln,
 *                                  AffineAlignBuffers& b)          (AffineOneGapAlign.h:157)
 * for n independent (q,t,k) problems.  Sequences are ASCII bytes inside device buffers
 * d_qseq / d_tseq (may be the same buffer); problem p uses d_qseq[q_off[p] .. +q_len[p]) and
 * d_tseq[t_off[p] .. +t_len[p]).
 * Outputs per problem: the returned score; the gapless blocks the reference appends to
 * aln.blocks, as (qPos,tPos,length) int32 triples written at d_blocks + 3*d_block_off[p]
 * (capacity d_block_off[p+1]-d_block_off[p] triples; min(q_len,t_len)+1 always suffices);
 * their count; a status word (bits above).                                              */
int lra_affine_one_gap_align_batch(lra_ctx* ctx, int n, const char* d_qseq, const char* d_tseq,
                                   const uint64_t* d_q_off, const int32_t* d_q_len,
                                   const uint64_t* d_t_off, const int32_t* d_t_len,
                                   const int32_t* d_k, int m, int mm, int indel,
                                   int32_t* d_score, int32_t* d_nblocks, int32_t* d_blocks,
                                   const uint64_t* d_block_off, int32_t* d_status);
/* Which of its kernels lra_affine_one_gap_align_batch gives a problem -- the classification arithmetic the device code itself calls, run on the
 * host: no context, no GPU, host arrays in and out.  For n problems of lengths q_len[p] x t_len[p] and band k[p] under the scoring (m, mm, indel):
 * cls_out[p] = the size class (0-9: the anti-diagonal sweep over score matrices in LDS, 2 and 6 the same in an HBM work slot of 4 / 8 MiB; 10-12: scores
 * in registers; 14-18: one lane per problem), or -1 where the batch call answers LRA_ST_RANGE; path_out[p] = the form of that class's kernel, bits
 * below (0 where cls_out[p] is -1).  Diagnostic: what the tests use to aim inputs at every form and at both sides of every size limit.          */
#define LRA_AOG_PATH_SUFFIX 1          /* the length difference exceeds the band: second (suffix) band and the long gap ("alignTop")    */
#define LRA_AOG_PATH_SCORES_MASK 6     /* where the prefix band's scores live during the sweep:                                         */
#define LRA_AOG_PATH_SCORES_LDS 0      /*   the flat matrices (classes 0-9 but 2, 6) or the lane kernel's previous row, in LDS          */
#define LRA_AOG_PATH_SCORES_REGS 2     /*   registers, two diagonals per lane (classes 10-12; 2 / 6 with k + 2 <= 64)                   */
#define LRA_AOG_PATH_SCORES_ROLLING 4  /*   three rotating anti-diagonal windows in LDS (classes 2 / 6)                                 */
#define LRA_AOG_PATH_SCORES_HBM 6      /*   the flat matrices in the HBM work slot (classes 2 / 6)                                      */
#define LRA_AOG_PATH_CODES_LDS 8       /* the sequence codes the sweep reads are in LDS (else: in the HBM work slot)                    */
int lra_aog_class_of_batch(int n, const int32_t* q_len, const int32_t* t_len, const int32_t* k, int m, int mm, int indel,
                           int32_t* cls_out, int32_t* path_out);

/* ---- a13 (DP leaf): the alignment between two consecutive chain anchors -------------------------------------
 * Replaces   RefineByLinearAlignment(btc_curReadEnd, btc_curGenomeEnd, btc_nextReadStart, btc_nextGenomeStart, str, chromIndex,
 *                                    alignment, read, genome, strands, ...)                    (LocalRefineAlignment.h:141-185)
 * = SetMatchAndGaps (:93) + RefineSubstrings (:127) + AlignSubstrings (:100) for n anchor pairs: if min(nextReadStart - curReadEnd + 1,
 * nextGenomeStart - curGenomeEnd + 1) > 0 and (opts.refineLevel & REF_DP), AffineOneGapAlign on strands[str][curReadEnd, nextReadStart)
 * x genome.seqs[chromIndex][curGenomeEnd, nextGenomeStart) with band min(2 * |qLen - tLen| + 1, opts.localBand); its blocks, shifted by
 * (curReadEnd, curGenomeEnd), are what the reference appends to alignment->blocks.  d_q_base[p] / d_t_base[p]: offset of strands[str] /
 * genome.seqs[chromIndex] inside d_qseq / d_tseq.  Output (context-owned): blocks CSR by pair (qPos,tPos,length), score, status
 * (AffineOneGapAlign bits; LRA_ST_RANGE if a span is negative).  Synchronous.                                                  */
typedef struct lra_between_result {
  uint64_t n_gaps, n_blocks;
  const uint64_t* d_block_off; const int32_t* d_blocks; const int32_t* d_score; const uint32_t* d_status;
} lra_between_result;
int lra_between_anchors_batch(lra_ctx* ctx, int n, const char* d_qseq, const uint64_t* d_q_base, const uint32_t* d_cur_read_end,
                              const uint32_t* d_next_read_start, const char* d_tseq, const uint64_t* d_t_base, const uint32_t* d_cur_genome_end,
                              const uint32_t* d_next_genome_start, int match, int mismatch, int indel, int local_band, int refine_dp,
                              lra_between_result* out);

/* ---- a13: the chain walk that turns the second sparse DP's chains into alignments ------------------------------------------------
 * Replaces   LocalRefineAlignment(ultimatechains, ext_clusters, alignments, smallOpts, LookUpTable, read, strands, h, genome, LSC, tinyOpts,
 *                                 buff, svsigstrm)                                   (LocalRefineAlignment.h:885-1029, Map_lowacc.h:576)
 * including RefinedAlignmentbtwnAnchors (:203-550) for n_jobs primary chains.  Job j (primary chain h = d_job_h[j] of read d_job_read[j]) has
 * the chains d_job_chain_off[j] .. d_job_chain_off[j+1] (ultimatechains[st], after RemovePairedIndels / RemoveSpuriousAnchors); chain c has
 * the anchors d_chain_anchor_off[c] .. (q on the forward read, t chromosome-relative, length; chain order = trace-back order), its cluster's
 * strand and chromIndex, FirstSDPValue, NumOfAnchors0, NumOfAnchors1.  d_strands = the reads forward, then (at rc_base) reverse complemented.
 * opts = tinyOpts: localW / globalW / localMaxFreq on entry, localMatch / localMismatch / localIndel / localBand, RefineBySDP, readType
 * (is_ont: clr / ont vs contig / ccs), and the PWL parameters of the sparse DP.
 * Output (context-owned): the SegAlignments each job pushes, in order: alignments d_job_aln_off[j] .. d_job_aln_off[j+1], each with strand,
 * Supplymentary, ISsecondary, NumOfAnchors0 / 1, chromIndex, value and its blocks (qPos, tPos, length) d_block_off[a] .. d_block_off[a+1].
 * d_status[j] != 0: the reference would read outside an array on that job (LRA_ST_OOB_SLOT: an empty inner chain; LRA_ST_RANGE: two anchors
 * that overlap on the read by two or more bases, a string of negative length in the reference); its alignments are then not defined.  Synchronous. */
typedef struct lra_lra_opts {
  int32_t localW, globalW, localMaxFreq, match, mismatch, indel, localBand, refineBySDP, isOnt;
  float gapopen, gapextend, gaproot; int32_t gapCeiling1, gapCeiling2;
} lra_lra_opts;
typedef struct lra_alignments_result {
  uint64_t n_jobs, n_alignments, n_blocks, n_big, n_inner_jobs;
  const uint64_t* d_job_aln_off;
  const int32_t* d_strand; const int32_t* d_supp; const int32_t* d_secondary; const int32_t* d_n0; const int32_t* d_n1; const int32_t* d_chrom; const float* d_value;
  const uint64_t* d_block_off; const int32_t* d_blocks; const uint32_t* d_status;
} lra_alignments_result;
int lra_local_refine_batch(lra_ctx* ctx, uint64_t n_jobs, const uint64_t* d_job_chain_off, const uint32_t* d_job_read, const int32_t* d_job_h, uint64_t n_chains,
                           const uint64_t* d_chain_anchor_off, const int32_t* d_chain_strand, const int32_t* d_chain_chrom, const float* d_chain_value,
                           const int32_t* d_chain_n0, const int32_t* d_chain_n1, uint64_t n_anchors, const uint32_t* d_q, const uint32_t* d_t, const int32_t* d_len,
                           const uint64_t* d_read_off, const char* d_strands, uint64_t rc_base, const char* d_genome, const uint64_t* h_chrom_pos, int n_chrom,
                           const lra_lra_opts* opts, lra_alignments_result* out);

/* The walk of the high-accuracy overload  LocalRefineAlignment(Primary_chains, splitchains, ExtendClusters, alignments, smallOpts, LookUpTable, read, strands,
 * p, h, genome, LSC, tinyOpts, buff, svsigstrm, extend_clusters, false)  (LocalRefineAlignment.h:577-766, Map_highacc.h:708) behind its sparse DP, filters and
 * SwitchToOriginalAnchors (:563-576): as lra_local_refine_batch, except that chain st of a job is splitchains[st] (pass empty chains for pieces whose
 * ultimatechain is empty), a chain of one anchor still makes an alignment (:579), Supplymentary = (st != d_job_lsc[job]), d_chain_value /
 * d_chain_n0 = Primary_chains[p].chains[h].value / NumOfAnchors0, d_chain_n1 = the chain's size.                                              */
int lra_local_refine_highacc_batch(lra_ctx* ctx, uint64_t n_jobs, const uint64_t* d_job_chain_off, const uint32_t* d_job_read, const int32_t* d_job_h,
                                   const uint32_t* d_job_lsc, uint64_t n_chains, const uint64_t* d_chain_anchor_off, const int32_t* d_chain_strand,
                                   const int32_t* d_chain_chrom, const float* d_chain_value, const int32_t* d_chain_n0, const int32_t* d_chain_n1, uint64_t n_anchors,
                                   const uint32_t* d_q, const uint32_t* d_t, const int32_t* d_len, const uint64_t* d_read_off, const char* d_strands, uint64_t rc_base,
                                   const char* d_genome, const uint64_t* h_chrom_pos, int n_chrom, const lra_lra_opts* opts, lra_alignments_result* out);

/* From the second sparse DP to lra_local_refine_batch (Map_lowacc.h:530-540, :575): `second` = lra_sparse_dp_batch in single-cluster mode over the
 * merged clusters of `merge`; its chains are filtered (RemovePairedIndels<UltimateChain>, RemoveSpuriousAnchors) and grouped per primary chain.
 * job = chain slot of the first sparse DP (read = slot / num_aln, h = slot % num_aln; d_slot_n0[slot] = chains[p].NumOfAnchors0 kept by the caller, the
 * first DP's result arrays being overwritten by the second; may be NULL), chains = its merged clusters.  Output (context-owned) = the array
 * arguments of lra_local_refine_batch.  Synchronous.                                                                                         */
typedef struct lra_local_refine_inputs {
  uint64_t n_jobs, n_chains, n_anchors;
  const uint64_t* d_job_chain_off; const uint32_t* d_job_read; const int32_t* d_job_h;
  const uint64_t* d_chain_anchor_off; const int32_t* d_chain_strand; const int32_t* d_chain_chrom; const float* d_chain_value; const int32_t* d_chain_n0;
  const int32_t* d_chain_n1; const uint32_t* d_q; const uint32_t* d_t; const int32_t* d_len;
} lra_local_refine_inputs;
int lra_local_refine_inputs_batch(lra_ctx* ctx, int num_aln, const uint32_t* d_slot_n0, const lra_merge_result* merge, const lra_chain_result* second,
                                  lra_local_refine_inputs* out);

/* ---- a14: banded 3-state affine indel refinement ----------------------------------------
 * Replaces   void IndelRefineAlignment(Read& read, Genome& genome, Alignment& alignment,
 *                                      const Options& opts, IndelRefineBuffers& buffers,
 *                                      bool endAlign = false)            (IndelRefine.h:53)
 * for n_aln alignments.  Alignment a: its gapless blocks alignment.blocks as (qPos,tPos,length)
 * int32 triples d_blocks_in[3*d_block_off[a] .. 3*d_block_off[a+1]) (absolute read / chromosome
 * coordinates); alignment.read = the read strand it is on = d_qseq + d_q_off[a] of length
 * d_q_len[a] (read.length); genome.seqs[alignment.chromIndex] = d_tseq + d_t_off[a] of length
 * d_t_len[a] (genome.lengths[chromIndex]).  refine_band = opts.refineBand, match /
 * mismatch / indel = opts.localMatch / localMismatch / localIndel, end_align as the argument.
 * refine_band must lie in 2..64 and indel must be negative; otherwise the call returns
 * LRA_ERR_INVALID before it launches anything, and out is left as it was.
 * Output: the refined alignment.blocks of every alignment (CSR, device arrays owned by the
 * context, valid until the next call), a status word per alignment (bits above; LRA_ST_RANGE
 * also flags a segment whose row window is wider than 1024 cells, the widest row the fill
 * kernels take).  Synchronous.                                                               */
typedef struct lra_refine_result {
  int32_t n_aln;
  uint64_t n_blocks, n_segments, n_rows, n_cells, n_aog;
  const uint64_t* d_block_off;   /* [n_aln+1] */
  const int32_t* d_blocks;       /* [3*n_blocks] */
  const int32_t* d_status;       /* [n_aln] */
} lra_refine_result;
int lra_indel_refine_batch(lra_ctx* ctx, int n_aln, const int32_t* d_blocks_in, const uint64_t* d_block_off,
                           uint64_t n_blocks_in, const char* d_qseq, const uint64_t* d_q_off,
                           const int32_t* d_q_len, const char* d_tseq, const uint64_t* d_t_off,
                           const int64_t* d_t_len, int refine_band, int match, int mismatch, int indel,
                           int end_align, lra_refine_result* out);

/* ---- a16: alignment statistics + CIGAR ---------------------------------------------------
 * Replaces   void Alignment::CalculateStatistics(const Options&, ostream*, const vector<float>& LookUpTable)
 * (Alignment.h:513-531 = CreateAlignmentStrings :247 + AlignStringsToCigar :414, opts.showmm) for
 * n_aln alignments given as blocks (same conventions as lra_indel_refine_batch; d_t_off is the
 * chromosome start).  h_lookup = the reference's LookUpTable (LogLookUpTable.h: logf(1), logf(6), ...,
 * 2001 floats, computed by the HOST libm so the float value matches the reference bit for bit).
 * Output per alignment: 18 int32 counters in the order
 *   nm nmm nins ndel tdel tins nSmallDel nMedDel nLargeDel nSmallIns nMedIns nLargeIns preClip sufClip qStart qEnd tStart tEnd
 * named after the reference's MEMBERS after the call (so nins counts deletion runs and ndel insertion
 * runs), the float `value` (NV), and the CIGAR as runs (length << 4 | op,
 * op 0 '=', 1 'X', 2 'I', 3 'D'), CSR by alignment.  Counters are this call's increments of a fresh
 * Alignment (the reference never resets tdel/tins/nSmall*).  Synchronous.                          */
typedef struct lra_stats_result {
  int32_t n_aln;
  uint64_t n_runs;
  const int32_t* d_counts;    /* [18*n_aln] */
  const float* d_value;       /* [n_aln] */
  const uint64_t* d_run_off;  /* [n_aln+1] */
  const uint32_t* d_runs;     /* [n_runs] */
} lra_stats_result;
int lra_calculate_statistics_batch(lra_ctx* ctx, int n_aln, const int32_t* d_blocks, const uint64_t* d_block_off,
                                   const char* d_qseq, const uint64_t* d_q_off, const int32_t* d_q_len,
                                   const char* d_tseq, const uint64_t* d_t_off, const float* h_lookup, int n_lookup,
                                   lra_stats_result* out);

/* ---- a17 (opts.printMD): the MD:Z value of every alignment, on the device --------------------------------------------
 * Replaces  CreateAlignmentStrings (Alignment.h:247-331) + AlignmentStringsToMD (:204-245)  on the final blocks, byte for byte what
 * lra_md_string(lra_alignment_strings(...)) gives: the columns compared as upper-cased characters (not seqMap: a read's N against a
 * reference A is a mismatch), insertions consumed silently, '^' + the reference run for a deletion, no number behind a trailing mismatch
 * or deletion, the empty string for an alignment without columns.  Arguments as lra_calculate_statistics_batch (d_q_len is not read).
 * Output (context-owned, valid until the next call on the context): alignment a's text at d_md + d_md_off[a], d_md_off[a + 1] - d_md_off[a]
 * bytes, no terminators; n_bytes = d_md_off[n_aln].  Synchronous.                                                                      */
typedef struct lra_md_result {
  int32_t n_aln;
  uint64_t n_bytes;
  const uint64_t* d_md_off;   /* [n_aln+1] */
  const char* d_md;           /* [n_bytes] */
} lra_md_result;
int lra_md_strings_batch(lra_ctx* ctx, int n_aln, const int32_t* d_blocks, const uint64_t* d_block_off, const char* d_qseq, const uint64_t* d_q_off,
                         const int32_t* d_q_len, const char* d_tseq, const uint64_t* d_t_off, lra_md_result* out);

/* ---- opts.Printsvsig / opts.svsigLen: the SV signatures of every alignment, on the device -----------------------------
 * Replaces  Alignment::Printsvsig (Alignment.h:336-411), which CalculateStatistics calls (:518) to fill MapRead's svsigstrm.  For every block b
 * of an alignment but the last: q / t = the block's end in the read / the chromosome, qg / tg = the bases from there to block b + 1, less their
 * common part min(qg, tg).  qg > min_len is one INS signature {t, t, qg, read[q, q + qg)}; otherwise tg > min_len is one DEL signature
 * {t, t + tg - 1, tg, text[t, t + tg)} -- the gap sits in front of the common columns.  read = d_qseq + d_q_off[a] (the strand the alignment lies
 * on), text = d_tseq + d_t_off[a] (its chromosome); positions are 0-based in the chromosome, bytes are copied as stored.  A pair with a negative
 * gap gives nothing (the reference asserts; the pipeline produces none).  Arguments as lra_md_strings_batch (d_q_len is not read), min_len >= 0.
 * Output (context-owned, valid until the next call on the context): alignment a's signatures are d_sig[d_sig_off[a] .. d_sig_off[a + 1]), in
 * block order; a signature's bases are d_seq[seq_off, seq_off + len), the sequences back to back in signature order.  Synchronous.            */
#define LRA_SV_INS 0
#define LRA_SV_DEL 1
typedef struct lra_svsig_rec {
  uint64_t seq_off;           /* of its bases in d_seq */
  uint32_t t_start;           /* t: the end of block `block` in the chromosome (INS: start = end = t; DEL: end = t + len - 1) */
  uint32_t len;               /* the net gap = the number of bases */
  uint32_t kind;              /* LRA_SV_INS / LRA_SV_DEL */
  uint32_t block;             /* the gap is behind this block of the alignment */
} lra_svsig_rec;
typedef struct lra_svsig_result {
  int32_t n_aln;
  uint64_t n_sig, n_seq_bytes;
  const uint64_t* d_sig_off;        /* [n_aln+1] */
  const lra_svsig_rec* d_sig;       /* [n_sig] */
  const char* d_seq;                /* [n_seq_bytes] */
} lra_svsig_result;
int lra_sv_signatures_batch(lra_ctx* ctx, int n_aln, const int32_t* d_blocks, const uint64_t* d_block_off, const char* d_qseq, const uint64_t* d_q_off,
                            const int32_t* d_q_len, const char* d_tseq, const uint64_t* d_t_off, int32_t min_len, lra_svsig_result* out);
/* The text of these signatures (MapRead's svsigstrm), on the device (svsig_text.hip).  sv: a result as lra_sv_signatures_batch leaves it.  Per
 * alignment: d_aln_read[a] its read, d_chrom[a] its chromosome, d_skip[a] (d_skip NULL: none) 1 when the alignment prints nothing.  The names are two
 * tables on the device, a blob and offsets each: read r's name is d_read_names[d_read_name_off[r], d_read_name_off[r + 1]), n_reads + 1 offsets; the
 * chromosomes' the same way (an index outside its table prints an empty name).  One line per signature, alignments in index order, an alignment's
 * signatures in d_sig order, each exactly what lra_map_svsig_host writes:
 *     chrom \t readName \t t_start \t end \t len \t INS|DEL \t bases \n
 * end = t_start for INS, (uint32)(t_start + len - 1) for DEL; decimal without padding; bases = d_seq[seq_off, seq_off + len) as stored.
 * Output (context-owned, valid until the next call on the context): alignment a's lines are d_text[d_aln_off[a], d_aln_off[a + 1]), n_bytes =
 * d_aln_off[n_aln]; nothing is written behind d_text + n_bytes.  n_sig == 0 launches nothing (d_aln_off is zeros, d_text NULL).  LRA_ERR_INVALID: a
 * NULL sv, negative counts, a NULL array or name table with n_sig > 0.  Synchronous.                                                          */
typedef struct lra_svsig_text_result {
  int32_t n_aln;
  uint64_t n_sig, n_bytes;
  const uint64_t* d_aln_off;        /* [n_aln+1] */
  const char* d_text;               /* [n_bytes] */
} lra_svsig_text_result;
int lra_svsig_text_batch(lra_ctx* ctx, const lra_svsig_result* sv, const uint32_t* d_aln_read, const int32_t* d_chrom, const uint8_t* d_skip, int n_reads,
                         const char* d_read_names, const uint64_t* d_read_name_off, int n_chrom, const char* d_chrom_names, const uint64_t* d_chrom_name_off,
                         lra_svsig_text_result* out);

/* ---- a17: the CIGAR strings of every alignment, on the device ----------------------------------------------------------
 * Replaces  the CIGAR field as Alignment::PrintSAM / PrintPAF write it (Alignment.h:640-650, :700-714): the clip in front (preClip, when > 0, and the
 * clip op), the runs CalculateStatistics left ((length << 4) | op, op 0..3 = "=XID"; lra_calculate_statistics_batch's d_runs / d_run_off), each as its
 * decimal length and its op, the clip behind (sufClip, when > 0).  d_pre_clip / d_suf_clip: per alignment, either may be NULL (no such clip; a clip
 * <= 0 prints nothing); d_clip_op: per alignment 'S' or 'H' (NULL: 'S').  An alignment without runs and without clips has the empty string.
 * Output (context-owned, valid until the next call on the context): alignment a's text at d_text + d_off[a], d_off[a + 1] - d_off[a] bytes, no
 * terminators; n_bytes = d_off[n_aln]; nothing is written behind d_text + n_bytes.  Synchronous.  The device record stage (lra_map_records_device)
 * builds every alignment's runs once with it, without clips: the same text goes into the alignment's own record and into the SA:Z of its group's
 * other segments, under different clip ops.                                                                                                     */
typedef struct lra_cigar_text_result {
  int32_t n_aln;
  uint64_t n_bytes;
  const uint64_t* d_off;      /* [n_aln+1] */
  const char* d_text;         /* [n_bytes] */
} lra_cigar_text_result;
int lra_cigar_text_batch(lra_ctx* ctx, int n_aln, const uint32_t* d_runs, const uint64_t* d_run_off, const int32_t* d_pre_clip, const int32_t* d_suf_clip,
                         const uint8_t* d_clip_op, lra_cigar_text_result* out);

/* ---- a17 (print format 'a'): the alignment strings and the pairwise text of every alignment, on the device (pairwise.hip) ----------------
 * Replaces  CreateAlignmentStrings (Alignment.h:247-331) and the rows of PrintPairwise (:564-589)  on the final blocks.  Arguments as
 * lra_md_strings_batch (d_q_len is not read).
 * lra_alignment_strings_batch: alignment a's three strings are d_q / d_a / d_t + d_col_off[a], d_col_off[a + 1] - d_col_off[a] bytes each, byte for byte
 * what lra_alignment_strings gives (pair columns carry '|' or '*' by seqMap equality, the net query gap comes first with ' ' over '-', then the net text
 * gap, then the gaps' common stretch as pair columns; characters as stored); d_ref_len[a] = Alignment::refLen as lra_alignment_strings leaves it: the
 * last block's tPos + length, 0 without blocks.  n_cols = d_col_off[n_aln].
 * lra_pairwise_text_batch: alignment a's text at d_text + d_off[a], d_off[a + 1] - d_off[a] bytes: what lra_format_pairwise writes behind the name line
 * and the "Interval:" line (first_q / first_t = the first block's qPos / tPos), 46 * ceil(c / 50) + 3 c bytes for c columns, built straight from the
 * blocks without the strings.  n_bytes = d_off[n_aln]; nothing is written behind d_text + n_bytes.
 * Outside the contract (the contents are unspecified, nothing is read or written out of range): blocks that overlap -- a negative length or gap, which
 * the reference asserts on and the pipeline does not make; a literal '-' in a read or a chromosome (the host form counts a row's coordinates from the
 * characters).  Output context-owned, valid until the next call on the context (n_aln == 0: LRA_OK, no arrays).  Synchronous.                        */
typedef struct lra_aln_strings_result {
  int32_t n_aln;
  uint64_t n_cols;
  const uint64_t* d_col_off;  /* [n_aln+1] */
  const uint32_t* d_ref_len;  /* [n_aln] */
  const char* d_q;            /* [n_cols] each */
  const char* d_a;
  const char* d_t;
} lra_aln_strings_result;
int lra_alignment_strings_batch(lra_ctx* ctx, int n_aln, const int32_t* d_blocks, const uint64_t* d_block_off, const char* d_qseq, const uint64_t* d_q_off,
                                const int32_t* d_q_len, const char* d_tseq, const uint64_t* d_t_off, lra_aln_strings_result* out);
typedef struct lra_pairwise_text_result {
  int32_t n_aln;
  uint64_t n_bytes;
  const uint64_t* d_off;      /* [n_aln+1] */
  const char* d_text;         /* [n_bytes] */
} lra_pairwise_text_result;
int lra_pairwise_text_batch(lra_ctx* ctx, int n_aln, const int32_t* d_blocks, const uint64_t* d_block_off, const char* d_qseq, const uint64_t* d_q_off,
                            const int32_t* d_q_len, const char* d_tseq, const uint64_t* d_t_off, lra_pairwise_text_result* out);

/* ---- a15: junctions of split alignments ---------------------------------------------------------------------
 * Replaces   RefineBreakpoint(read, genome, leftAln, rightAln, opts)   (RefineBreakpoint.h:210-466; Map_lowacc.h:592, Map_highacc.h:725)
 * for n junctions: if the read bases between the two segments (in forward read coordinates) number 1..499, both segments are extended into
 * the gap by a full DP (RSdp: match 2, mismatch -2, gap -4), cut where the summed score is best, and the new blocks are glued on
 * (PrependBlocks / AppendBlocks).  Per junction and side: the segment's blocks (CSR, (qPos,tPos,length) triples), its strand, the offset
 * of Alignment::read (the read strand it is aligned on) in d_seq, the offset and length of its chromosome in d_genome; d_read_len.
 * Output (context-owned): the two block lists after the call, at d_*_blocks + 3 * d_*_off[j] with d_*_n[j] blocks each; status bit
 * 0x10000 = refined, LRA_ST_OOB_SLOT = the reference would read outside the read / chromosome (lists unchanged).  Synchronous.   */
typedef struct lra_breakpoint_result {
  uint64_t n_junctions;
  const int32_t* d_l_blocks; const uint64_t* d_l_off; const int32_t* d_l_n;
  const int32_t* d_r_blocks; const uint64_t* d_r_off; const int32_t* d_r_n;
  const uint32_t* d_status;
} lra_breakpoint_result;
int lra_refine_breakpoint_batch(lra_ctx* ctx, int n, const int32_t* d_read_len, const char* d_seq, const char* d_genome, const int32_t* d_l_blocks,
                                const uint64_t* d_l_off, const int32_t* d_l_strand, const uint64_t* d_l_read_off, const uint64_t* d_l_chrom_off,
                                const int32_t* d_l_chrom_len, const int32_t* d_r_blocks, const uint64_t* d_r_off, const int32_t* d_r_strand,
                                const uint64_t* d_r_read_off, const uint64_t* d_r_chrom_off, const int32_t* d_r_chrom_len, lra_breakpoint_result* out);

/* ---- a17: SAM / PAF / BED records (host code, no device work) ------------------------------------------
 * Byte-for-byte the text of  Alignment::PrintSAM (Alignment.h:658-808), SimplePrintSAM (:811-905), PrintPAF (:600-656) and
 * PrintBed (:591-598) for alignments described by plain records (the fields those functions read).  Tags in the reference's order:
 * SAM  NM MM NX ND TD NI TI NV AS AO N0 RT TP SD ME LD SI MI LI [SA];  simple SAM  RT NM NX ND TD NI TI N0 NV AS AO;
 * PAF  OR NM NX ND TD NI TI SD ME LD SI MI LI N0 NV AS TP [NA] [RT] [CG].  opts.printMD: rec.md (NULL: no tag) is printed as MD:Z after LI by
 * lra_format_sam only, as the reference does (SimplePrintSAM, PrintPAF and PrintBed print no MD); lra_map_records_host fills it from a
 * snapshot packed with LRA_PACK_MD.  n_blocks == 0 prints the unaligned record.  lra_format_sam prints segment `as` of the group and lists the other
 * segments, last to first, in SA:Z.  passthrough: the text appended when opts.passthroughtag is set (NULL otherwise).
 * Output: at most cap bytes into out (no terminator); *len = bytes needed.  Returns LRA_ERR_INVALID if cap < *len.            */
typedef struct lra_aln_record {
  const char* read_name; const char* read; const char* qual;   /* qual: NULL, "*" or read_len quality characters (NUL-terminated) */
  int32_t read_len;
  const char* chrom; uint32_t genome_len;                      /* Alignment::chrom, genomeLen */
  const char* cigar;
  uint32_t flag; int32_t strand; uint32_t mapqv; int32_t supplementary, typeofaln;
  uint32_t q_start, q_end, t_start, t_end; int32_t pre_clip, suf_clip;
  int32_t nm, nmm, nins, ndel, tdel, tins, nSmallDel, nMedDel, nLargeDel, nSmallIns, nMedIns, nLargeIns;
  float value; int32_t order, NumOfAnchors0, NumOfAnchors1, runtime;
  int32_t n_blocks; uint32_t first_block_qpos, last_block_qend;   /* blocks[0].qPos and blocks[last].qPos + length (hard-clipped substrings) */
  int32_t is_secondary;                                        /* Alignment::ISsecondary (read by lra_group_alignments, not printed) */
  const char* md;                                              /* NULL, or the MD:Z value (opts.printMD; lra_md_string) */
  /* print format 'a' (PrintPairwise) only, NULL otherwise: the blocks, Alignment::read (the read on the alignment's strand) and a pointer p
   * with p[tPos] = chromosome base tPos for every tPos the blocks cover */
  const int32_t* blocks; const char* strand_read; const char* chrom_text;
} lra_aln_record;
int lra_format_sam(const lra_aln_record* group, int n_group, int as, int hard_clip, const char* passthrough, char* out, uint64_t cap, uint64_t* len);
int lra_format_sam_simple(const lra_aln_record* rec, int hard_clip, const char* passthrough, char* out, uint64_t cap, uint64_t* len);
int lra_format_paf(const lra_aln_record* rec, int print_cigar, char* out, uint64_t cap, uint64_t* len);
int lra_format_bed(const lra_aln_record* rec, char* out, uint64_t cap, uint64_t* len);
/* "@PG\tID:lra\tPN:lra\tVN:<version>\tCL:<command_line>" (lra.cpp:665-671) + one "@SQ\tSN:..\tLN:.." per chromosome (Genome.h:85-89) */
int lra_format_sam_header(const char* version, const char* command_line, const char* const* chrom_names, const uint64_t* chrom_pos, int n_chrom,
                          char* out, uint64_t cap, uint64_t* len);

/* Alignment strings and what is printed from them (host code): CreateAlignmentStrings (Alignment.h:247-331), AlignmentStringsToMD (:204-245,
 * the MD:Z value PrintSAM adds with opts.printMD), PrintPairwise (:564-589, print format "a").  Two-call convention as above.             */
int lra_alignment_strings(const char* query, const char* text, const int32_t* blocks, int n_blocks, char* q_out, char* a_out, char* t_out, uint64_t cap,
                          uint64_t* len, uint32_t* ref_len);
int lra_md_string(const char* query_str, const char* ref_str, uint64_t n, char* out, uint64_t cap, uint64_t* len);
int lra_format_pairwise(const char* read_name, const char* chrom, int n_blocks, int first_q, int first_t, uint32_t ref_len, const char* query_str,
                        const char* align_str, const char* ref_str, uint64_t n, char* out, uint64_t cap, uint64_t* len);

/* ---- a16 / a17: a read's alignments between CalculateStatistics and the text records (host code) -------------------------------
 * lra_group_alignments  = SegAlignmentGroup::SetFromSegAlignment (Alignment.h:944-983) for n_groups alignments whose segment records are
 *                         recs[seg_off[g] .. seg_off[g+1]) (SegAlignment order): sums, flags (REVERSE, SUPPLEMENTARY), ISsecondary.
 * lra_order_alignments  = AlignmentsOrder::Update (:1021-1046; operator() :1048, std::sort): index[old_end..n_groups) ordered by
 *                         (value, NumOfAnchors0) descending, first primary, others secondary (SECONDARY flag, typeofaln 2 unless 3).
 * lra_simple_mapqv      = SimpleMapQV (Mapping_ultility.h:497-595), opts.bypassClustering / readType == clr / == ont / globalK.
 * lra_output_read       = OUTPUT (:453-493) and output_unaligned (:445-451): formats 's' (PrintSAM), 'b' (PrintBed), 'p' / 'P' (PrintPAF
 *                         without / with CIGAR), 'a' (PrintPairwise; needs the records' blocks / strand_read / chrom_text); sets Alignment::order;
 *                         two-call convention of the lra_format_* functions.                                                             */
typedef struct lra_aln_group {
  int32_t first, count;
  uint32_t q_start, q_end, t_start, t_end; int32_t nm, nmm, ndel, nins; int32_t is_secondary; float value; int32_t NumOfAnchors0, NumOfAnchors1;
} lra_aln_group;
int lra_group_alignments(lra_aln_record* recs, const int32_t* seg_off, int n_groups, lra_aln_group* groups);
int lra_order_alignments(lra_aln_group* groups, int n_groups, lra_aln_record* recs, int32_t* index, int old_end);
int lra_simple_mapqv(const lra_aln_group* groups, const int32_t* index, int n_groups, lra_aln_record* recs, int bypass_clustering, int is_clr, int is_ont,
                     int globalK);
int lra_output_read(const lra_aln_group* groups, const int32_t* index, int n_groups, lra_aln_record* recs, int print_num_aln, char format, int hard_clip,
                    const char* passthrough, int read_unaligned, const lra_aln_record* unaligned_rec, char* out, uint64_t cap, uint64_t* len);

/* ---- a7 (high-accuracy path): MergeMatchesSameDiag -----------------------------------------------------------------------------------
 * Replaces   MergeMatchesSameDiag(extend_clusters, samediag_clusters, opts)                    (LinearExtend.h:795-829, Map_highacc.h:642)
 * for n_clusters extended clusters: cluster c has the anchors d_anchor_off[c] .. d_anchor_off[c+1] (read pos, chromosome pos, length,
 * Cluster::overlap flag, in the cluster's order) and its strand.  Output: Cluster_SameDiag::start / end of cluster c =
 * d_start / d_end [d_group_off[c] .. d_group_off[c+1]) (anchor indices relative to the cluster); d_status[c] = LRA_ST_OOB_SLOT for an
 * empty cluster (the reference reads matches[0]).  Synchronous.                                                                        */
typedef struct lra_same_diag_result {
  uint64_t n_clusters, n_groups;
  const uint64_t* d_group_off; const uint32_t* d_start; const uint32_t* d_end; const uint32_t* d_status;
} lra_same_diag_result;
int lra_merge_same_diag_batch(lra_ctx* ctx, uint64_t n_clusters, const uint64_t* d_anchor_off, const uint32_t* d_q, const uint32_t* d_t,
                              const int32_t* d_len, const uint8_t* d_overlap, const int32_t* d_strand, int merge_dist, lra_same_diag_result* out);

/* ---- a11 (high-accuracy path): RefineBtwnSpace --------------------------------------------------------------------------------------
 * Replaces   int RefineBtwnSpace(int K, int W, vector<Cluster>& RevBtwnCluster, bool twoblocks, Cluster* cluster, const Options& opts, Genome&, Read&,
 *                                char* strands[2], GenomePos qe, GenomePos qs, GenomePos te, GenomePos ts, bool st, GenomePos lrts = 0,
 *                                GenomePos lrlength = 0)                                   (ClusterRefine.h:331-432; caller RefineBtwnClusters_chain :433)
 * for n spaces, up to the vector insert + SetClusterBoundariesFromMatches it ends with (the caller owns the clusters): per space the read it
 * belongs to, cluster->chromIndex, qs / qe / ts / te (t relative to the chromosome) and st as the caller passes them, twoblocks, lrts / lrlength
 * (NULL = 0).  read_type = LRA_READ_* (opts.readType picks refineSpaceDiag), anchorstoosparse / match / mismatch / indel / max_freq =
 * opts.anchorstoosparse / localMatch / localMismatch / localIndel / localMaxFreq.  Output per space: d_decision 0 nothing (:371), 1 the
 * pairs go into the cluster (:363-369), 3 the same after the reverse strand was tried (:415-421: anchorfreq = 1 too), 2 the pairs form a
 * new RevBtwnCluster on the other strand (:422-431, the reference returns 1); the pairs (CSR), refine efficiencies eff / reff (-1 when the
 * reverse strand was not tried).  Synchronous.                                                                                           */
typedef struct lra_btwn_space_result {
  uint64_t n, n_pairs, n_reverse_tried;
  const uint64_t* d_pair_off; const uint32_t* d_pair_q; const uint32_t* d_pair_t; const int32_t* d_decision; const float* d_eff; const float* d_reff;
} lra_btwn_space_result;
int lra_refine_btwn_space_batch(lra_ctx* ctx, int n, const uint32_t* d_qs, const uint32_t* d_qe, const uint32_t* d_ts, const uint32_t* d_te, const int32_t* d_st,
                                const uint8_t* d_twoblocks, const uint32_t* d_read, const int32_t* d_chrom, const uint32_t* d_lrts, const uint32_t* d_lrlength,
                                const uint64_t* d_read_off, const char* d_strands, uint64_t rc_base, const char* d_genome, const uint64_t* h_chrom_pos, int n_chrom,
                                int K, int W, int read_type, float anchorstoosparse, int match, int mismatch, int indel, int max_freq,
                                lra_btwn_space_result* out);

/* ---- a11 (high-accuracy path): RefineBtwnClusters_chain -------------------------------------------------------------------------------
 * Replaces   for every chain (p, h) of a read, in order: RefineBtwnClusters_chain(K, W, Primary_chains, RefinedClusters, RevBtwnCluster, tracerev,
 *            genome, read, smallOpts, p, h, strands)                               (ClusterRefine.h:433-614, Map_highacc.h:513-518)
 * Reads: d_read_chain_off[n_reads+1] over the chains (a read's chains in the reference's order); chain x = cluster indices
 * d_ch[d_chain_off[x] .. d_chain_off[x+1]) in the chain's order (ch[0] nearest the read's end).  Clusters (the RefinedClusters of the batch): matches
 * CSR d_match_off over d_mq / d_mt (t relative to the chromosome), d_box {qStart, qEnd, tStart, tEnd} = SetClusterBoundariesFromMatches of those
 * matches for K (UPDATED IN PLACE), d_strand, d_chrom, d_anchorfreq (UPDATED IN PLACE: 1 where RefineBtwnSpace decided on the cluster's own
 * strand after trying both, :414-419).  K / W: what the caller passes on (Map_highacc.h:466-468); read_type, anchorstoosparse, match, mismatch,
 * indel, max_freq as lra_refine_btwn_space_batch.  d_strands: the reads forward, then (at rc_base) reverse complemented.
 * Output (context-owned): every cluster's matches with the refined spaces' pairs appended in the reference's order (CSR), Cluster::refinespace.
 * Synchronous.                                                                                                                              */
typedef struct lra_btwn_clusters_result {
  uint64_t n_clusters, n_matches, n_problems, n_pairs_added; uint32_t n_rounds;
  const uint64_t* d_match_off; const uint32_t* d_q; const uint32_t* d_t; const uint8_t* d_refinespace;
} lra_btwn_clusters_result;
int lra_refine_btwn_clusters_batch(lra_ctx* ctx, int n_reads, const uint64_t* d_read_chain_off, uint64_t n_chains, const uint64_t* d_chain_off, const uint32_t* d_ch,
                                   uint64_t n_clusters, const uint64_t* d_match_off, uint64_t n_matches, const uint32_t* d_mq, const uint32_t* d_mt, uint32_t* d_box,
                                   const int32_t* d_strand, const int32_t* d_chrom, float* d_anchorfreq, const uint64_t* d_read_off, const char* d_strands, uint64_t rc_base,
                                   const char* d_genome, const uint64_t* h_chrom_pos, int n_chrom, int K, int W, int read_type, float anchorstoosparse, int match, int mismatch,
                                   int indel, int max_freq, lra_btwn_clusters_result* out);

/* ---- a9 (high-accuracy path): SPLITChain over merged clusters -----------------------------------------------------------------------------
 * Replaces   SPLITChain(read, ExtendClusters, splitchains, Primary_chains[p].chains[h].link, smallOpts)   (Mapping_ultility.h:266-346, Map_highacc.h:706)
 * including MergeSplitchainINS (:172-262) and LargestSplitChain_dist (Chain.h:974-985, Map_highacc.h:707) for n_jobs chains.  Job j = the
 * Cluster_SameDiag elements d_job_off[j] .. d_job_off[j+1] (strand 0 = forward, chromIndex, box = qStart, qEnd, tStart, tEnd with t relative to
 * the chromosome) and the link bits d_link[d_link_off[j] ..] (entry im joins elements im and im + 1).  splitdist = opts.splitdist.
 * Output (context-owned): pieces of job j = d_job_piece_off[j] .. d_job_piece_off[j+1]; piece p = the elements d_sptc[d_piece_off[p] ..
 * d_piece_off[p+1]) (indices inside the job, in SplitChain::sptc order), its type ('T' 'D' 'I' 'N'), Strand, box (QStart, QEnd, TStart, TEnd);
 * d_job_lsc[j] = LSC.  The reference leaves chromIndex of a chain's last piece indeterminate (Chain.h:350-360): it compares unequal to
 * every other piece's here.  Synchronous.                                                                                                  */
typedef struct lra_hsplit_result {
  uint64_t n_jobs, n_pieces, n_elems;
  const uint64_t* d_job_piece_off; const uint64_t* d_piece_off; const uint32_t* d_sptc; const uint8_t* d_piece_type; const uint8_t* d_piece_strand;
  const uint32_t* d_piece_box; const uint32_t* d_piece_job; const uint32_t* d_job_lsc;
} lra_hsplit_result;
int lra_split_chains_highacc_batch(lra_ctx* ctx, uint64_t n_jobs, const uint64_t* d_job_off, uint64_t n_elems, const int32_t* d_strand, const int32_t* d_chrom,
                                   const uint32_t* d_box, const uint64_t* d_link_off, const uint8_t* d_link, int splitdist, lra_hsplit_result* out);

/* ---- GlobalChain / PrioritySearchTree (named by the path's description; not reachable from lra.cpp) -------------------------------------------
 * Replaces   int GlobalChain(vector<Fragment>& fragments, vector<int>& optFragmentChainIndices, vector<Endpoint>& endpoints)   (GlobalChain.h:85-189,
 *            PrioritySearchTree.h; called by TestGlobalChain.cpp:17 only)
 * for n_sets independent fragment sets: set s = fragments d_off[s] .. d_off[s+1] (xl, yl, xh, yh, initial score -- TestGlobalChain.cpp:14 uses xh - xl).
 * Output (context-owned): per fragment its final score and prev (index inside the set, -1 = none); per set the optimal chain's fragment indices
 * d_chain[d_off[s] .. d_off[s] + d_chain_len[s]).  Synchronous.                                                                                  */
typedef struct lra_global_chain_result {
  uint64_t n_sets, n_fragments;
  const int32_t* d_score; const int32_t* d_prev; const int32_t* d_chain; const uint32_t* d_chain_len;
} lra_global_chain_result;
int lra_global_chain_batch(lra_ctx* ctx, uint64_t n_sets, const uint64_t* d_off, uint64_t n_fragments, const int32_t* d_xl, const int32_t* d_yl, const int32_t* d_xh,
                           const int32_t* d_yh, const int32_t* d_score, lra_global_chain_result* out);

/* ---- a13 helper (high-accuracy path): SwitchToOriginalAnchors ------------------------------------------------------------------------
 * Replaces   SwitchToOriginalAnchors(finalchain, ultimatechain, ExtendClusters, extend_clusters)      (LocalRefineAlignment.h:187-199, :576)
 * for n_chains chains over Cluster_SameDiag entries: chain c = elements d_chain_off[c] .. d_chain_off[c+1], element i = entry d_elem_entry[i]
 * of cluster d_elem_cluster[i] (FinalChain::chain / ClusterNum); same_diag = the lra_merge_same_diag_batch result the entries refer to;
 * d_coarse[cluster] = Cluster_SameDiag::coarse.  Output: per chain the original anchors (index inside their cluster, entry by entry from its
 * last anchor to its first) and their ClusterIndex, at d_chain_off[c] .. d_chain_off[c+1] of the result.  Synchronous.                   */
typedef struct lra_original_anchors_result {
  uint64_t n_chains, n_anchors;
  const uint64_t* d_chain_off; const uint32_t* d_anchor; const int32_t* d_cluster;
} lra_original_anchors_result;
int lra_switch_to_original_anchors_batch(lra_ctx* ctx, uint64_t n_chains, const uint64_t* d_chain_off, uint64_t n_elems, const int32_t* d_elem_cluster,
                                         const uint32_t* d_elem_entry, const lra_same_diag_result* same_diag, const int32_t* d_coarse,
                                         lra_original_anchors_result* out);

/* ---- a9 (high-accuracy path): switchindex ---------------------------------------------------------------------------------------------
 * Replaces   switchindex(splitclusters, Primary_chains, clusters, genome, read)                (Mapping_ultility.h:39-168, Map_highacc.h:274)
 * for n_chains chains (every CHain of every Primary_chain of every read): chain c = d_ch[d_chain_off[c] .. d_chain_off[c+1]) (split-cluster
 * indices relative to its read, as lra_sparse_dp_boxes_batch returns them) with d_n_link[c] link bits at d_link[d_chain_off[c] ..];
 * d_split_base[c] / d_cluster_base[c] = where its read's split clusters (d_coarse) / clusters (d_cl_qs, d_cl_qe = Cluster::qStart, qEnd)
 * begin; n_total = d_chain_off[n_chains].  Output (context-owned, same offsets): the rewritten chain d_ch[d_chain_off[c] .. + d_n[c]) of
 * cluster indices and d_n_link[c] links; d_status[c] = LRA_ST_OOB_SLOT where the reference would index past a vector.  Synchronous.     */
typedef struct lra_switchindex_result {
  uint64_t n_chains;
  const uint32_t* d_ch; const uint8_t* d_link; const uint32_t* d_n; const uint32_t* d_n_link; const uint32_t* d_status;
} lra_switchindex_result;
int lra_switchindex_batch(lra_ctx* ctx, uint64_t n_chains, const uint64_t* d_chain_off, const uint32_t* d_ch, const uint8_t* d_link,
                          const uint32_t* d_n_link, const uint64_t* d_split_base, const uint64_t* d_cluster_base, const int32_t* d_coarse,
                          const uint32_t* d_cl_qs, const uint32_t* d_cl_qe, uint64_t n_total, lra_switchindex_result* out);

/* ---- the path behind one call: MapRead_lowacc for a batch of reads -----------------------------------------------------------------
 * Replaces   int MapRead_lowacc(const vector<float>& LookUpTable, Read& read, Genome& genome, vector<GenomeTuple>& genomemm, LocalIndex& glIndex,
 *                               const Options& opts, ostream* output, ostream* svsigstrm, Timing& timing, IndelRefineBuffers&, pthread_mutex_t*)
 *            (Map_lowacc.h:33-640), which MapRead (MapRead.h:153-263) enters for the low-accuracy presets (-ONT, -CLR), called by the MapReads
 *            worker (lra.cpp:117) and the serial loop (lra.cpp:721) once per read.
 * The reference side (shared, read-only in the reference too) is loaded once per context:
 *   lra_ctx_load_genome        genome.seqs back to back                                  (Genome.h:122-137)
 *   lra_ctx_load_chromosomes   genome.header.pos, n_chrom + 1 cumulative starts          (Genome.h:60-83)
 *   lra_ctx_load_global_index  genomemm, the .mms payload                                (MMIndex.h:416)
 *   lra_ctx_build_local_index  glIndex: LocalIndex::IndexSeq of every chromosome on the device (the .gli payload; MMIndex.h:200-254)
 * lra_map_reads_lowacc_batch aligns n_reads reads (d_seq: upper-case bases back to back, >= 64 bytes of padding behind the last read;
 * d_read_off: n_reads + 1 offsets; total_bases = d_read_off[n_reads]) and leaves, in context-owned buffers valid until the next call:
 *   job j = read j / num_aln, primary chain j % num_aln (the loop over chains, Map_lowacc.h:232); its SegAlignments are alignments
 *   d_job_aln_off[j] .. d_job_aln_off[j+1] (empty when the chain produced none); per alignment: read, strand, Supplymentary, ISsecondary,
 *   NumOfAnchors0 / 1, chromIndex, FirstSDPValue (value before CalculateStatistics), the refined blocks (IndelRefineAlignment),
 *   CalculateStatistics' 18 counters (order of lra_calculate_statistics_batch), NV value and CIGAR runs ((length << 4) | op, op in =XID).
 *   d_job_status[j] != 0 / d_refine_status[a] != 0: the reference would read outside an array there (see the stage headers).
 * lra_map_records is the per-read tail (SetFromSegAlignment, AlignmentsOrder::Update, SimpleMapQV, OUTPUT / output_unaligned,
 * Map_lowacc.h:600-618) on the host: text of all reads in input order, two-call convention; rec_off (nullable): n_reads + 1 offsets of
 * each read's records inside the text.  names / reads / quals (nullable, or NULL / "*" entries) / read_len: per read, host.            */
#define LRA_READ_ONT 0
#define LRA_READ_CLR 1
#define LRA_READ_CCS 2
#define LRA_READ_CONTIG 3
typedef struct lra_map_opts {
  int32_t globalK, globalW, globalMaxFreq;
  int32_t localK, localW, localMaxFreq, localIndexWindow;
  int32_t refineBand, localMatch, localMismatch, localIndel, localBand;
  int32_t refineSpaceDist; float anchorstoosparse; int32_t splitdist, window;
  float second_anchorbonus; int32_t bypassClustering, skipBandedRefine, refineBreakpoint;   /* refineBreakpoint: --refineBreakpoints (lra.cpp:262) */
  lra_clean_opts clean; lra_sdp_opts sdp;
  int32_t readType, hardClip, PrintNumAln, printFormat;   /* printFormat: 's' SAM, 'p' / 'P' PAF, 'b' BED, 'a' pairwise (PrintPairwise) */
  lra_fine_opts fine; int32_t merge_dist;                 /* high-accuracy path only: MatchesToFineClusters, MergeMatchesSameDiag */
  int32_t defer_matches;                                  /* low-accuracy path, scheduling only (results do not depend on it): a read with more refined matches than this
                                                           * after Refine_Btwnsplitchain goes on in a second, concurrent pass; 0 = one pass (the presets) */
  int32_t flagged_unaligned;                              /* what lra_map_records* write for a read whose status word is non-zero (an LRA_ST_* condition in some stage: the
                                                           * result is not known to equal the reference's): 0 (the presets) = an empty record, the caller re-runs those reads
                                                           * elsewhere (counters.n_flagged_reads / lra_map_host_flagged say how many and which); 1 = the read's unaligned
                                                           * record (output_unaligned, Mapping_ultility.h:457-463: a flag-4 line in SAM mode), so that the output keeps one
                                                           * record per input read */
  int32_t defer_seed_matches;                             /* low-accuracy path, scheduling only (a read's result does not depend on the batch it is mapped in): a read with
                                                           * more tier-1 matches than this (CompareLists against the global index; a 30 kb read has ~3 k, a read from a
                                                           * satellite array 6-10 k) is HANDED BACK: it leaves the batch behind the seed stage, d_read_status[r] has
                                                           * LRA_ST_DEFERRED (and nothing else), counters.n_handed_back_reads counts them, lra_map_records* write nothing
                                                           * for it.  The caller collects such reads and maps them as batches of their own (with this field 0): their
                                                           * sparse DPs are tens of times larger than a typical read's and would otherwise set the length of every
                                                           * latency-bound launch of the batch they sit in.  0 = off (the presets) */
} lra_map_opts;
typedef struct lra_map_counters {
  uint64_t n_minimizers, n_matches, n_clusters, n_sdp_anchors, n_sdp_points, n_sdp_entries, n_local_tuples, n_local_tasks, n_local_task_words, n_local_pairs, n_refined_matches,
           n_btwn_problems, n_btwn_rounds, n_refined_after_btwn, n_merged_clusters, n_sdp2_anchors, n_sdp2_entries, n_a13_blocks, n_large_spaces, n_segments,
           n_rows, n_cells, n_aog, n_deferred_reads,
           n_flagged_reads,                                  /* reads of the batch with a non-zero d_read_status (no alignment record is written for them) */
           n_handed_back_reads;                              /* (ABI 6) reads handed back UNMAPPED by the seed stage under opts.defer_seed_matches (status LRA_ST_DEFERRED, no record):
                                                              * what a caller sizes its pool of handed-back reads with.  n_deferred_reads counts only the reads that opts.defer_matches
                                                              * moved to the batch's second pass -- those ARE mapped and have their records */
} lra_map_counters;
typedef struct lra_map_result {
  int32_t n_reads, num_aln;
  uint64_t n_jobs, n_alignments, n_blocks, n_runs;
  const uint64_t* d_job_aln_off; const uint32_t* d_job_status;
  const uint8_t* d_job_reached;     /* [n_jobs] 1: primary chain p reached Map_lowacc.h:574 (its SegAlignmentGroup exists, possibly empty).  The reference's loop over p ENDS at
                                     * the first chain that does not (p > 0: break, :267 / :491; p == 0: the read is unaligned): the low-accuracy driver maps no chain behind
                                     * it (their flags are 0, they have no alignments).  One rule is left to the reader of these arrays, as lra_map_records* apply it: a read
                                     * whose chain 0 reached :574 but got no SegAlignment is unaligned whatever its later chains hold (:578-581) */
  const uint32_t* d_read_status;    /* [n_reads] OR of every stage's LRA_ST_* bits for the read; non-zero = not bit-identical, no record is emitted */
  const uint32_t* d_aln_read; const int32_t* d_strand; const int32_t* d_supp; const int32_t* d_secondary; const int32_t* d_n0; const int32_t* d_n1;
  const int32_t* d_chrom; const float* d_first_sdp_value;
  const uint64_t* d_block_off; const int32_t* d_blocks; const int32_t* d_refine_status;
  const int32_t* d_counts; const float* d_value; const uint64_t* d_run_off; const uint32_t* d_runs;
  const char* d_strands; uint64_t rc_base;                 /* the reads forward, then (at rc_base) reverse complemented; the drivers leave the batch's read
                                                            * offsets [n_reads + 1] behind them, at byte (2 * rc_base + 64 + 7) & ~7 (what LRA_PACK_MD addresses
                                                            * the reads with: the caller's d_read_off may be reused by then) */
  lra_map_counters counters;
} lra_map_result;
void lra_map_opts_preset_ont(lra_map_opts* opts);          /* -ONT: lra.cpp:386-431 over Options.h:127-230 */
void lra_map_opts_preset_clr(lra_map_opts* opts);          /* -CLR: lra.cpp:341-386 */
int lra_ctx_load_chromosomes(lra_ctx* ctx, const uint64_t* h_chrom_pos, int n_chrom);
int lra_ctx_build_local_index(lra_ctx* ctx, int k, int w, int window, int max_freq);
/* glIndex's k, w and localIndexWindow belong to the INDEX, not to the options: LocalIndex::Read takes them from the .gli file (MMIndex.h:154-173, lra.cpp:627), the reads'
 * indexes copy them (LocalIndex(LocalIndex&), MMIndex.h:128-136, Map_lowacc.h:246-247) and smallOpts.globalK / globalW are glIndex.k / w (Map_lowacc.h:233-234,
 * Map_highacc.h:430-431).  `lra index` writes k = 10, w = 5, windows of 2048 bases under EVERY preset (`LocalIndex glIndex;` lra.cpp:989 -> LocalIndex(0): 1 <<
 * (LOCAL_POS_BITS - 1), MMIndex.h:110-127; RunStoreLocal keeps k = 10, lra.cpp:785-817), so an `lra align` run on indexed files maps with those; only without a .gli file
 * does it build glIndex from opts.localK (10 for -ONT / -CLR, 7 for -CCS / -CONTIG) and opts.localIndexWindow = 256 (lra.cpp:619-621, :628) -- the values the presets
 * below hold.  lra_map_opts_apply_local_index writes an index's three values into the options (localK, localW, localIndexWindow); lra_ctx_local_index_params returns the
 * ones the context's index was built with.  The drivers refuse options that differ from the context's index (LRA_ERR_INVALID).                                        */
void lra_map_opts_apply_local_index(lra_map_opts* opts, int k, int w, int window);
/* glIndex as LocalIndex::Read left it (MMIndex.h:154-173, lra.cpp:627): the .gli payload handed over as it is (host arrays, copied) instead of lra_ctx_build_local_index --
 * glIndex.k / w / localIndexWindow, seqOffsets[n_windows + 1], tupleBoundaries[n_windows + 1], minimizers[n_tuples].  The seqOffsets must be those IndexSeq writes for the
 * loaded chromosome table at this window (an index of another genome is LRA_ERR_INVALID).                                                                            */
int lra_ctx_load_local_index(lra_ctx* ctx, int k, int w, int window, uint64_t n_windows, const uint64_t* h_seq_offsets, const uint64_t* h_tuple_bnd,
                             uint64_t n_tuples, const uint32_t* h_tuples);
int lra_ctx_local_index_params(lra_ctx* ctx, int* k, int* w, int* window);
/* The context's reference data as device pointers: the genome bytes; the genome's local index (the .gli payload: d_tuple_bnd[n_windows + 1],
 * d_tuples[n_tuples]) and its seqOffsets[n_windows + 1].  Valid until the context is destroyed or the data is loaded / built again.        */
/* Several contexts on one GPU (sub-batches on their own HIP streams) share ONE replica of the reference: dst borrows src's genome, global
 * index, chromosome table and local index; src must outlive dst; dst must not hold reference data of its own.                              */
int lra_ctx_share_reference(lra_ctx* dst, lra_ctx* src);
const char* lra_ctx_genome_ptr(lra_ctx* ctx);
int lra_ctx_local_index(lra_ctx* ctx, lra_local_index_result* out, const uint64_t** d_seq_offsets);
int lra_map_reads_lowacc_batch(lra_ctx* ctx, int n_reads, const char* d_seq, const uint64_t* d_read_off, uint64_t total_bases, const lra_map_opts* opts,
                               lra_map_result* out);
/* Two-stage batches (low-accuracy presets): lra_map_reads_lowacc_batch in two halves, so that the FRONT half of batch i + 1 runs beside the BACK half of batch i.
 *   front: a1 .. the second LinearExtend / TrimOverlappedAnchors (Map_lowacc.h:69-476), on `ctx` and its stream, by one host thread;
 *   back : the second sparse DP, LocalRefineAlignment, IndelRefineAlignment, CalculateStatistics (Map_lowacc.h:477-599), on the context's companion context
 *          (made on first use: its own stream -- the device's highest priority unless LRA_BACK_PRIORITY says otherwise --, its own work buffers, the reference data shared), by ANOTHER host thread.
 * Between the halves sits a queue of ONE batch (ABI 6; before: none -- the front half waited for the running back half): the front half writes what it hands over
 * into one of two sets of handover buffers, taken in turn, and lra_map_reads_lowacc_front returns when the batch is handed over; it waits, at its very end, only until
 * the batch BEFORE its own has been taken by a back call -- the back half that is running is not waited for, so the back context goes from one batch straight to the
 * next.  lra_map_reads_lowacc_back waits for a handed-over batch, runs its back half and returns the result of the whole batch exactly as lra_map_reads_lowacc_batch
 * would (same alignments, same counters); the result's arrays belong to *back_ctx: lra_map_pack / lra_map_snapshot / lra_map_records are called on THAT context, then
 * lra_map_back_release(ctx) ends the result's lifetime (the next back call needs it: LRA_ERR_INVALID while a result is held).  Up to three batches are in flight (one in
 * its back half, one handed over, one in its front half): a batch's reads (d_seq, d_read_off) stay untouched until ITS back call has returned.  Per thread the calls are
 * in batch order: front(0), front(1), ... on one, back(0), release(0), back(1), ... on the other.  Scheduling only; opts.defer_matches and opts.defer_seed_matches do not
 * combine with it (LRA_ERR_INVALID).  The reference's counterpart is its pool of worker threads (lra.cpp:678-714): several reads in flight at different points of MapRead.
 * Errors (ABI 6): a front call that FAILS -- whatever the reason: reference not loaded, out of memory, a stage's error -- still hands over a batch, an ERROR batch: the
 * back call that takes it runs nothing, returns the front call's code and holds nothing (NO lra_map_back_release for it; one would return LRA_ERR_INVALID).  So the
 * contract for the two host threads is one back call per front call, whatever either returned; the thread of the back halves is never left waiting for a batch that
 * does not come, and the next front call is not blocked by a failed one.  A back call whose own half fails returns its code with the result slot still held: release
 * it as after a success.  The back calls leave their error text on the back context (lra_ctx_last_error(*back_ctx); the front thread owns ctx's).
 * The back context's view of the reference data (borrowed from ctx) is refreshed by each back call before it runs, on its own thread; ctx's reference must not be
 * loaded / built again while a batch is in flight (the halves in flight read it). */
int lra_map_reads_lowacc_front(lra_ctx* ctx, int n_reads, const char* d_seq, const uint64_t* d_read_off, uint64_t total_bases, const lra_map_opts* opts);
int lra_map_reads_lowacc_back(lra_ctx* ctx, const lra_map_opts* opts, lra_map_result* out, lra_ctx** back_ctx);
int lra_map_back_release(lra_ctx* ctx);

/* The same boundary for the high-accuracy presets: MapRead_highacc (Map_highacc.h:37-798) behind MapRead (MapRead.h:169-239), which the reference enters
 * when opts.bypassClustering == 0 (-CCS, -CONTIG).  Arguments and result as lra_map_reads_lowacc_batch; job j = read j / num_aln, chain h = j % num_aln of
 * Primary_chains[0] (num_aln = opts.NumAln); d_job_reached[j] = the chain has clusters and got its SegAlignmentGroup (:697-699); d_first_sdp_value =
 * Primary_chains[0].chains[h].value.  The counters of CalculateStatistics are what the reference's two calls (:721, :731) leave: tdel, tins and the six size
 * classes accumulate over both.  Needs the genome, the chromosome table and the global index; the genome's local index only when a read takes the REFINEclusters
 * branch (:413-447: a second pass over those reads with K = glIndex.k, merged into the result; their d_job_reached carries bit 1).  lra_map_records / lra_map_snapshot / lra_map_pack serve both paths
 * (opts.bypassClustering tells the record stage which tail to follow).                                                                          */
void lra_map_opts_preset_ccs(lra_map_opts* opts);          /* -CCS: lra.cpp:306-340 */
void lra_map_opts_preset_contig(lra_map_opts* opts);       /* -CONTIG: lra.cpp:268-305 */
int lra_map_reads_highacc_batch(lra_ctx* ctx, int n_reads, const char* d_seq, const uint64_t* d_read_off, uint64_t total_bases, const lra_map_opts* opts,
                                lra_map_result* out);
/* ---- the input side ---------------------------------------------------------------------------------------------------
 * lra_reads_open / lra_reads_next_batch / lra_reads_close replace Input::Initialize, Input::GetNext (FASTA and FASTQ) and Input::BufferedRead (Input.h:87-168,
 * :182-283, :405-421): files are read one after the other; a batch takes reads while it holds fewer than max_bases bases (so it ends with the read that
 * crosses the limit).  The batch's arrays are owned by the reader and valid until the next call: seq = the reads' bases, upper-cased, back to back + 64 bytes
 * of padding; off[n_reads + 1]; names / reads / quals / read_len as lra_map_records takes them (quals[i] == NULL for FASTA reads).
 * A FASTQ record whose quality string has another length than its read (the reference asserts, Input.h:287) makes lra_reads_next_batch return LRA_ERR_INVALID
 * on that call and on every later one: the batch of that call holds the reads in front of the record, lra_reads_last_error names the record.
 * lra_map_reads_host is the boundary with host buffers: it copies the batch to the device and calls the driver opts->bypassClustering selects.
 * SAM (plain or BGZF-compressed) and BAM files are read as GetNext's HTS branch reads them (Input.h:296-393), without htslib: records whose flag meets
 * lra_reads_set_flag_remove's mask are skipped (-Flag), the bases are the 4-bit codes through "=ACMGRSVTWYHKDBN", the qualities +33; a record without
 * qualities has quals[i] == NULL.  Where the reference's input stops without a word -- a truncated file, a bad BGZF block, a bad record, a SAM SEQ / QUAL
 * length mismatch, a file behind a SAM / BAM file (never read), a SAM / BAM file behind a FASTQ file that an empty batch would meet -- the call returns
 * LRA_ERR_INVALID as for a corrupt FASTQ record: lra_reads_last_error names the file and the reason (a block by its compressed offset, a record by its
 * index), the batch holds the reads in front of it, and the error is sticky.
 * lra_reads_open refuses compressed FASTA / FASTQ as the reference does.  lra_reads_open_flags(files, n, LRA_READS_COMPRESSED_TEXT, &r) (additive to
 * ABI 9; flags 0 = lra_reads_open) takes them, gzip and BGZF: a file that starts 1f 8b is sniffed by its inflated head with the FASTA / FASTQ rule, and a
 * compressed file yields exactly the batches its decompressed bytes would yield as a plain file at the same place in the file list (names, bases,
 * qualities, off, read_len, batch cuts, the FASTQ end-of-file rules, the quality-length error, what happens to the files behind it).  BGZF that holds BAM
 * or SAM stays BAM / SAM; other gzip that holds neither FASTA nor FASTQ (gzip'd SAM, gzip'd BAM bytes) stays refused.  A compression fault (a truncated
 * file, a bad code, a CRC-32 or ISIZE mismatch, bytes behind a member that start no member) follows the BAM reader's rule: LRA_ERR_INVALID, sticky, the
 * file and the member's compressed offset in lra_reads_last_error; the batch holds the records that are whole in the bytes in front of the fault.
 * The device form inflates BGZF members on the device (one wave per member) and parses where the data lies; gzip that is not BGZF is one serial bit
 * stream, inflated by ONE host thread in both forms (about 0.16 GB/s of text): BGZF is the format to use at speed.
 * Not supported: streamed input ("-", "stdin", "/dev/stdin": the format sniffing seeks; the reference refuses to stream SAM / BAM), CRAM, and gzip that is
 * not BGZF around anything but FASTA / FASTQ.  */
typedef struct lra_reads lra_reads;
typedef struct lra_read_batch {
  int32_t n_reads; uint64_t total_bases;
  const char* seq; const uint64_t* off; const int32_t* read_len;
  const char* const* names; const char* const* reads; const char* const* quals;
} lra_read_batch;
int lra_reads_open(const char* const* files, int n_files, lra_reads** out);
#define LRA_READS_COMPRESSED_TEXT 1   /* lra_reads_open_flags: gzip / BGZF FASTA and FASTQ files are read */
int lra_reads_open_flags(const char* const* files, int n_files, uint32_t flags, lra_reads** out);   /* flags outside the defined ones: LRA_ERR_INVALID */
int lra_reads_next_batch(lra_reads* r, uint64_t max_bases, lra_read_batch* batch);
const char* lra_reads_last_error(const lra_reads* r);
uint64_t lra_map_host_trim(uint64_t keep_bytes);   /* (ABI 6) the record stage keeps its threads' text parts between batches (process-wide, at most LRA_PARTS_POOL_MB, default 4096, of
                                                     * host memory; a fresh 100 MB part is 25 000 page faults): release them down to keep_bytes (0 = all); returns the bytes still held */
int lra_host_thread_budget(void);   /* host threads lra_map_records* use when asked for 0: hardware threads, capped by the container's CPU quota (cgroup cpu.max) less four */
void lra_reads_close(lra_reads* r);
/* lra_reads_next_batch with the parsing on ctx's device: the SAME batch (reads, cut, names, quals, errors) in *batch (host arrays, as lra_reads_next_batch
 * returns them), and the batch's bases / offsets on the device: *d_seq = the upper-cased bases back to back + 64 zero bytes, *d_off[n_reads + 1] with
 * d_off[0] = 0 -- what lra_map_reads_lowacc_batch / _highacc_batch / _lowacc_front take.  Device arrays are owned by the reader, work is enqueued on ctx's
 * stream and complete at return; both stay valid until the next call on r or lra_reads_close.  A reader uses one form: lra_reads_next_batch on a reader
 * that has used this one, or this one on a reader that has used lra_reads_next_batch, returns LRA_ERR_INVALID (this form reads ahead of its batches).
 * The reader's device buffers live on the device of its first call (another device: LRA_ERR_INVALID). */
int lra_reads_next_batch_device(lra_reads* r, lra_ctx* ctx, uint64_t max_bases, lra_read_batch* batch, const char** d_seq, const uint64_t** d_off);
/* bytes of a file the device form reads and parses per step (default 256 MiB; minimum 4096).  A step holds at least one whole record: one longer than
 * the step makes that step read on.  LRA_ERR_INVALID on a reader that has used lra_reads_next_batch. */
int lra_reads_set_device_chunk(lra_reads* r, uint64_t bytes);
/* -Flag and --passthrough of SAM / BAM input (lra.cpp:194, :246): both only before the first batch (after it: LRA_ERR_INVALID).  flags: records with
 * flag & flags != 0 are skipped.  on (0 / 1): lra_reads_batch_tags gives each SAM / BAM read of the last batch its aux fields as sam_format1 prints them
 * (the text behind its 11th tab: A as XX:A:c, every integer type as XX:i:<decimal>, f as XX:f:%g, Z and H as written, B as XX:B:<t>,v1,v2...; fields
 * joined by tabs), NULL for a read without aux fields.  *tags[n_reads] is owned by the reader, valid until the next call; every entry is NULL for
 * FASTA / FASTQ reads and when passthrough is off. */
int lra_reads_set_flag_remove(lra_reads* r, uint32_t flags);
int lra_reads_set_passthrough(lra_reads* r, int on);
int lra_reads_batch_tags(const lra_reads* r, const char* const** tags);
/* What a batch of lra_reads_next_batch_device keeps on the device besides its bases (additive to ABI 9; mode 0, the default, is the reader as it was).
 * Only before the first batch (after it: LRA_ERR_INVALID, as lra_reads_set_flag_remove); bits outside the two below: LRA_ERR_INVALID.  It is a setter and
 * no bit of lra_reads_open_flags, which refuses every flag but LRA_READS_COMPRESSED_TEXT as before.
 *   LRA_READS_DEV_QUAL     every batch also leaves its qualities on the device: lra_reads_batch_device_quals gives d_qual and d_qual_off[n_reads + 1], owned
 *                          by the reader and valid until the next call on r.  Read i's qualities are d_qual[d_qual_off[i], d_qual_off[i + 1]), as they are
 *                          in batch->quals[i]; the range is empty for a read without (FASTA, a BAM record with 0xff qualities, SAM '*') -- exactly what
 *                          lra_map_records_device takes as d_qual / d_qual_off (64 zero bytes lie behind the last string).  The bytes never touch the
 *                          host: every run of a step's records goes from the step's buffer to d_qual through lra_pack_strings_batch's kernel; records
 *                          the device form parses on the host (SAM text) have theirs uploaded into the same array.  A batch that ends in an error has
 *                          the ranges of exactly the reads it holds.  The host arrays of the batch are unchanged.  Cost: one byte of device memory per
 *                          base of the batch on top of d_seq (0.86 GB for a batch of 0.86 G bases).
 *   LRA_READS_DEV_NO_HOST  for a caller that reads neither the bases nor the qualities on the host (lra_map_records_device with formats 's' / 'P' / 'a').
 *                          Requires LRA_READS_DEV_QUAL (without it: LRA_ERR_INVALID).  The device-to-host copies of bases and qualities and the
 *                          page-locked buffers behind them are skipped: batch->seq is NULL, every batch->reads[i] is NULL, and batch->quals[i] is NULL
 *                          for a read without qualities, else a stub -- the string's first byte (none for an empty string) and a NUL, which is all
 *                          lra_map_records_device reads of it.  Names, off, read_len, tags, the batch cut and every error rule and text stay as they are.
 * lra_reads_batch_device_quals: LRA_ERR_INVALID on a reader without LRA_READS_DEV_QUAL, on one that uses lra_reads_next_batch, and before the first batch. */
#define LRA_READS_DEV_QUAL 1
#define LRA_READS_DEV_NO_HOST 2
int lra_reads_set_device_resident(lra_reads* r, uint32_t mode);
int lra_reads_batch_device_quals(const lra_reads* r, const char** d_qual, const uint64_t** d_qual_off);
/* n strings that lie anywhere in one device buffer, packed back to back (additive to ABI 9): string i is the d_dst_off[i + 1] - d_dst_off[i] bytes at
 * d_src + d_src_pos[i] and goes to d_dst + d_dst_off[i]; d_dst_off[n + 1] ascends from d_dst_off[0] = 0 (another value: LRA_ERR_INVALID).  Exactly
 * d_dst[0, d_dst_off[n]) is written.  Of the source, the aligned 4-byte words that hold a byte of a string are read and nothing else (a source range and
 * the destination must not overlap).  One wave per 4096 bytes of OUTPUT, whatever the strings' lengths: a string of 1 MB is 256 waves, 20 strings of 200
 * bytes are one.  n = 0 and empty strings are legal.  Device arrays, on ctx's device and stream, complete at return. */
int lra_pack_strings_batch(lra_ctx* ctx, uint64_t n, const char* d_src, const uint64_t* d_src_pos, const uint64_t* d_dst_off, char* d_dst);
/* BGZF inflate (the SAM/BAM spec's section 4.1; RFC 1951 / 1952), the stage the BAM reader runs: member i is in[in_off[i], in_off[i + 1]) -- a gzip
 * member with a 'BC' field whose BSIZE + 1 is its length --, its data goes to out[out_off[i], out_off[i + 1]), which must be its ISIZE (<= 65536).
 * status[i]: 0, or the reason the member is bad (1 header, 2 data ends early, 3 more than ISIZE, 4 invalid code, 5 distance before the block, 6 stored
 * LEN / NLEN, 7 less than ISIZE, 8 CRC-32, 9 ISIZE): nothing outside a member's ranges is read or written.  _batch: device arrays, on ctx's device and
 * stream, complete at return (one wave per member); _host: host arrays, the same decoder.  _lut_batch: the contract of _batch by the table-driven
 * kernel (inflate_lut.hip: lookup tables and an output ring in LDS, the whole wave copies matches and writes dwords), the compressed text reader's. */
int lra_bgzf_inflate_batch(lra_ctx* ctx, int n_blocks, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_out_off, uint8_t* d_out,
                           int32_t* d_status);
int lra_bgzf_inflate_lut_batch(lra_ctx* ctx, int n_blocks, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_out_off, uint8_t* d_out,
                               int32_t* d_status);
int lra_bgzf_inflate_host(int n_blocks, const uint8_t* in, const uint64_t* in_off, const uint64_t* out_off, uint8_t* out, int32_t* status);
/* BGZF deflate, the inverse stage (additive to ABI 9): member i is the data in[in_off[i], in_off[i + 1]) and becomes one complete BGZF member at
 * out + i * LRA_BGZF_SLOT -- the 18-byte header with the 'BC' field (BSIZE = the member's length - 1), raw DEFLATE data, CRC-32, ISIZE -- of out_len[i]
 * (<= 65536) bytes.  Data longer than LRA_BGZF_IN_MAX: status[i] != 0, out_len[i] = 0, nothing else written (a status per member, as inflate gives).
 * Length 0 gives a valid empty member; n_blocks = 0 is legal.  Nothing outside [slot, slot + out_len[i]) is written and nothing outside the member's
 * data is read (single bytes and unaligned words inside it: the input needs no alignment and no padding); the device form writes the slot in aligned
 * dwords, so d_out must be 4-byte aligned (else LRA_ERR_INVALID).  One algorithm, no level: a single-candidate hash of three bytes, greedy parse,
 * matches of 3 .. 258 at distances up to 32768 inside the member, dynamic Huffman blocks of 4096 positions, each written stored when that is not
 * smaller (65280 random bytes still fit the slot).  The parse is defined by position (lra_amd/csrc/bgzf_deflate.h states the rule), so _host and _batch
 * give byte-identical members, whatever a member's place in the batch, its alignment and its neighbours.  _batch: device arrays, on ctx's device and
 * stream, complete at return (one wave per member). */
#define LRA_BGZF_IN_MAX 65280   /* bytes of data per member (htslib's block size: a stored member of it still fits 64 KiB) */
#define LRA_BGZF_SLOT 65536     /* bytes a member may take */
int lra_bgzf_deflate_batch(lra_ctx* ctx, int n_blocks, const uint8_t* d_in, const uint64_t* d_in_off, uint8_t* d_out, uint32_t* d_out_len,
                           int32_t* d_status);
int lra_bgzf_deflate_host(int n_blocks, const uint8_t* in, const uint64_t* in_off, uint8_t* out, uint32_t* out_len, int32_t* status);
/* The stream stage: the device text d_text[0, len) cut every LRA_BGZF_IN_MAX bytes, deflated in rounds of a bounded number of members (the slots of a
 * round are the stage's scratch: 2048 members, 128 MiB, and as much for the round's packed members, whatever len is), each round's members packed back
 * to back (lra_pack_strings_batch's kernel) and copied into a page-locked buffer the context keeps.  *h_data[0, *data_len) holds the members,
 * member i at (*h_member_off)[i] .. [i + 1] (n_members + 1 entries); both are owned by the context and valid until the next call on it.  len = 0 gives
 * zero members; no EOF member is appended (the file's writer does that).  On ctx's device and stream, complete at return.
 *   lra_bgzf_compress_set_round   members per round (0: the default), for tests and for a caller short of device memory.
 *   lra_bgzf_compress_stats       the last call's wall time in ms and its output bytes (either may be NULL). */
int lra_bgzf_compress_device(lra_ctx* ctx, const uint8_t* d_text, uint64_t len, const uint8_t** h_data, uint64_t* data_len,
                             const uint64_t** h_member_off, uint64_t* n_members);
int lra_bgzf_compress_set_round(lra_ctx* ctx, int members);
int lra_bgzf_compress_stats(lra_ctx* ctx, double* ms_deflate, uint64_t* bgzf_bytes);
/* ---- the genome (Genome::Read, Genome.h:115-138) -------------------------------------------------------------------------------------------------
 * A genome FASTA file -- plain text, gzip or BGZF, as gzopen takes them -- into what lra_ctx_load_genome[_device] and lra_ctx_load_chromosomes take: the
 * bases of all records back to back, upper-cased, and header.pos.  The parsing rules are kseq_read's FASTA branch; lra_amd/csrc/genome.hip states them.
 * In short: bytes in front of the first '>' or '@' are dropped; a record starts at a line whose first byte is '>' or '@'; its name runs to the first
 * isspace byte (it may be empty); of a sequence line every byte is a base (blanks, tabs and digits too) but one '\r' in front of the '\n'; empty lines
 * are skipped; a record without bases is kept; a file without records gives n_chrom = 0 and LRA_OK.
 *   lra_genome_open          opens and sniffs the file: BGZF (a 'BC' field), other gzip (1f 8b 08), else plain text.  LRA_ERR_INVALID: no such file.
 *   lra_genome_read_host     parses everything on the host.
 *   lra_genome_read_device   parses on ctx's device, on ctx's stream, complete at return: the file is read in steps into page-locked memory and
 *                            parsed by byte-stream kernels; BGZF members are inflated on the device, other gzip on the host (one serial bit stream).
 *                            A reader uses one form (the other one afterwards: LRA_ERR_INVALID); a second call of the same form returns the first's code.
 *   lra_genome_info          after a read: the number of records, the bytes of their names (with the NULs), the number of bases.
 *   lra_genome_names         names[names_len]: the names NUL-terminated, back to back; pos[n_chrom + 1] = header.pos (either may be NULL).
 *   lra_genome_host_seq / lra_genome_device_seq   the bases, owned by the reader, + 64 zero bytes; NULL for the other form.
 *   lra_genome_install       lra_ctx_load_genome[_device] + lra_ctx_load_chromosomes from what the reader holds (device form: device to device, on
 *                            the reader's device).  A genome without records is LRA_ERR_INVALID here.
 *   lra_genome_set_device_chunk   bytes of the file's data per step (default 256 MiB, minimum 4096; before the read).  The host form decodes
 *                            compressed input in steps of the same size.
 * LRA_ERR_INVALID from a read, with lra_genome_last_error naming the place, and sticky: a line that starts with '+' inside a record (a FASTQ genome
 * is not read; the text names the record); a record whose first sequence line is "\r" alone (kseq would keep that '\r' as a base; refused); a bad
 * compressed member (named by its compressed offset: truncated, a bad code, CRC-32, ISIZE, bytes that start no member); 2^32 bases or more.  Of several
 * faults the first in file order is reported, by both forms alike.                                                                              */
typedef struct lra_genome lra_genome;
int lra_genome_open(const char* path, lra_genome** out);
int lra_genome_read_host(lra_genome* g);
int lra_genome_read_device(lra_genome* g, lra_ctx* ctx);
int lra_genome_info(const lra_genome* g, int32_t* n_chrom, uint64_t* names_len, uint64_t* total);
int lra_genome_names(const lra_genome* g, char* names, uint64_t* pos);
const char* lra_genome_host_seq(const lra_genome* g);
const char* lra_genome_device_seq(const lra_genome* g);
int lra_genome_install(const lra_genome* g, lra_ctx* ctx);
const char* lra_genome_last_error(const lra_genome* g);
int lra_genome_set_device_chunk(lra_genome* g, uint64_t bytes);
void lra_genome_close(lra_genome* g);
int lra_map_reads_host(lra_ctx* ctx, int n_reads, const char* h_seq, const uint64_t* h_off, const lra_map_opts* opts, lra_map_result* out);
int lra_map_records(lra_ctx* ctx, const lra_map_result* res, const lra_map_opts* opts, const char* const* names, const char* const* reads,
                    const char* const* quals, const int32_t* read_len, const char* const* chrom_names, const char* passthrough, char* out, uint64_t cap,
                    uint64_t* len, uint64_t* rec_off);
/* lra_map_records in two halves, so that the host tail of batch i runs beside the device side of batch i + 1 (the reference interleaves them per
 * thread, lra.cpp:117-158):
 *   lra_map_snapshot      copies what the records need (per-alignment fields, counters, CIGAR runs, block ends; with_blocks & LRA_PACK_BLOCKS also
 *                         every block and the chromosome text under it, needed by print format 'a' only; with_blocks & LRA_PACK_MD the MD:Z value
 *                         of every alignment, lra_md_strings_batch on the result's own arrays, which format 's' then prints -- opts.printMD;
 *                         with_blocks & LRA_PACK_SVSIG the SV signatures of every alignment, which lra_map_svsig_host prints -- opts.Printsvsig) from
 *                         the context's result buffers to a host object; after it returns the context may run the next batch.
 *   lra_map_records_host  SetFromSegAlignment / AlignmentsOrder::Update / SimpleMapQV / OUTPUT for every read on n_threads host threads (0: up to
 *                         16); touches neither the context nor the device.  *text (owned by the snapshot, valid until it is freed or reused),
 *                         *len bytes, (*rec_off)[n_reads + 1] record boundaries; a read with a non-zero status word has an empty record.
 *   lra_map_host_free     releases the snapshot.                                                                                              */
typedef struct lra_map_host lra_map_host;
#define LRA_PACK_BLOCKS 1   /* the flag word of lra_map_snapshot / lra_map_pack (0 / 1 as before): the blocks (print format 'a') */
#define LRA_PACK_MD 2       /* the MD:Z strings (opts.printMD): launches lra_md_strings_batch; the pack's header word 10 = their bytes, word 11 = 1 */
#define LRA_PACK_SVSIG 4    /* the SV signatures (opts.Printsvsig): launches lra_sv_signatures_batch with the context's svsig length
                             * (lra_ctx_set_svsig_len); the pack's header word 12 = the section's bytes, word 13 = 1.  The record text is unchanged */
#define LRA_PACK_NORUNS 8   /* leave the CIGAR runs out (the pack's header word 6 = 0, the runs section is empty; run_off stays): what lra_map_records_device
                             * copies -- its CIGAR text is built on the device.  lra_map_records_host on such a snapshot is LRA_ERR_INVALID when an alignment has runs */
int lra_map_snapshot(lra_ctx* ctx, const lra_map_result* res, int with_blocks, lra_map_host** out);
int lra_map_records_host(lra_map_host* snap, const lra_map_opts* opts, const char* const* names, const char* const* reads, const char* const* quals,
                         const int32_t* read_len, const char* const* chrom_names, const char* passthrough, int n_threads, const char** text, uint64_t* len,
                         const uint64_t** rec_off);
void lra_map_host_free(lra_map_host* snap);
/* lra_map_records / lra_map_records_host with one passthrough text per read (NULL: none), as lra_reads_batch_tags gives them: --passthrough of SAM /
 * BAM input (Alignment.h:797, :900).  The text of a read is that of the functions above with passthrough = passthrough[i]. */
int lra_map_records_tags(lra_ctx* ctx, const lra_map_result* res, const lra_map_opts* opts, const char* const* names, const char* const* reads,
                         const char* const* quals, const int32_t* read_len, const char* const* chrom_names, const char* const* passthrough, char* out,
                         uint64_t cap, uint64_t* len, uint64_t* rec_off);
int lra_map_records_host_tags(lra_map_host* snap, const lra_map_opts* opts, const char* const* names, const char* const* reads, const char* const* quals,
                              const int32_t* read_len, const char* const* chrom_names, const char* const* passthrough, int n_threads, const char** text,
                              uint64_t* len, const uint64_t** rec_off);
/* The record text built on the device.  For print formats 's' (SAM), 'P' (PAF with CG:z:) and 'a' (pairwise) *text, *len and (*rec_off)[n_reads + 1] are exactly what
 * lra_map_records_host_tags gives for a snapshot of the same result under the same options (flags & LRA_PACK_MD: with MD:Z, opts.printMD;
 * flags & LRA_PACK_SVSIG: the SV signature text is built too, see lra_map_records_device_svsig below; other flag bits are LRA_ERR_INVALID).  The
 * split of work:
 *   host    SetFromSegAlignment, AlignmentsOrder::Update, SimpleMapQV, the grouping and PrintNumAln, and every SHORT field of a record (name, flag,
 *           chrom, pos, MAPQ, the clips, the tag block with NV:f: through libstdc++, the short parts of SA:Z, passthrough text, the unaligned
 *           prefix), on n_threads threads (0: as lra_map_records_host) from a snapshot packed with LRA_PACK_NORUNS: the per-alignment arrays only --
 *           neither the CIGAR runs nor a base nor a quality is copied or touched.  The result is a PIECE TABLE: per record, in order, literals (ranges
 *           of one small blob) and references to long fields;
 *   device  the long fields: every alignment's CIGAR text (lra_cigar_text_batch, built once, copied into its own record and every SA:Z that names
 *           it), SEQ from the result's d_strands (forward, or at rc_base for a reverse-strand record; under -H a supplementary record's
 *           [q_start, q_end)), QUAL from d_qual (read r's qualities at d_qual + d_qual_off[r], d_qual_off[n_reads + 1], an empty range for a read
 *           without -- every non-NULL string of quals, as long as it is; a reverse-strand record's qualities stay as they came, Alignment.h:717-733; under -H a supplementary record's
 *           [first_block_qpos, last_block_qend), PrintSAM's own quirk), MD:Z from lra_md_strings_batch.  A count pass over the pieces, a scan, one
 *           copy pass cut by OUTPUT bytes, one device-to-host copy of the text into a page-locked buffer the context keeps.
 * quals (host, nullable, entries NULL or starting with '*': the field is "*") says which reads HAVE qualities; the host reads a string's first byte
 * only.  d_qual == NULL: the qualities of the reads that need them are uploaded from quals; a device reader with LRA_READS_DEV_QUAL hands over d_qual / d_qual_off
 * themselves (lra_reads_batch_device_quals), and with d_qual the host strings are not read behind their first byte.  reads (host) is read by the fall-through formats only and may be NULL for 's' / 'P' / 'a':
 * SEQ is the bases the batch was mapped from (d_strands), which the readers hand over upper-cased as they uploaded them.  passthrough: NULL, or one
 * text per read (NULL entries: none), as lra_map_records_tags takes them.  Flagged, handed-back and unaligned reads follow lra_map_records_host's rules
 * (an unaligned read's quality string is written as it is, a leading '*' too, as SimplePrintSAM does; one that is shorter than its read -- "*" -- is
 * written as far as it goes, where the host form reads read_len bytes whatever the string holds).
 * Print format 'a' (pairwise) is a device format too: per printed segment the name line and the "Interval:" line are host literals (from the counters
 * t_start / t_end the snapshot carries) and the rows are one piece, lra_pairwise_text_batch on the result's own blocks, strands and the genome (which must
 * be loaded) -- no block and no base crosses to the host; flags and quals are not used by this format; its limits are lra_pairwise_text_batch's.
 * Formats 'p' and 'b' have no long per-base field worth moving: the call falls through to lra_map_snapshot + lra_map_records_host_tags and returns that
 * text (in pageable memory).
 * *text / *rec_off are owned by the context and valid until the next lra_map_records_device on it; the result's arrays must still be alive (call it
 * where lra_map_snapshot would be called).  lra_map_records_device_last: where the last call's time and bytes went (zeros after a fall-through).
 * flags & LRA_PACK_SVSIG (opts.Printsvsig; alone or with LRA_PACK_MD; the record text is unchanged by it): the call also builds MapRead's second
 * stream and keeps it on the context, where lra_map_records_device_svsig returns it until the next lra_map_records_device: *text, *len and
 * (*rec_off)[n_reads + 1] are byte for byte what lra_map_svsig_host gives for lra_map_snapshot(ctx, res, LRA_PACK_SVSIG) of the same result (length
 * = lra_ctx_set_svsig_len; a read with a non-zero status word has no lines).  For the device formats it runs lra_sv_signatures_batch on the result's
 * own blocks, strands and the genome and lra_svsig_text_batch with d_aln_read, d_chrom, a skip byte made from d_read_status and the read and
 * chromosome names uploaded as blobs (a few tens of bytes per read); rec_off is gathered at the job offsets on the device and the text crosses in one
 * copy into a page-locked buffer the context keeps -- no signature record, block or base crosses to the host.  The fall-through formats take their
 * snapshot with the flag and print through lra_map_svsig_host.  LRA_ERR_INVALID when the last call on the context had no LRA_PACK_SVSIG (or there was
 * none). */
typedef struct lra_records_device_stats {
  double ms_snapshot;      /* pack without the runs + its device-to-host copy + unpack */
  double ms_cigar_md;      /* lra_cigar_text_batch (+ lra_md_strings_batch); format 'a': lra_pairwise_text_batch; BAM records: + the three lra_bam_* primitives */
  double ms_pieces;        /* the host's piece table (wall) */
  double ms_upload;        /* pieces, blob (+ qualities when they come from the host) */
  double ms_kernels;       /* resolve, scan, copy */
  double ms_copy_kernel;   /* of these: the copy pass alone (HIP events) */
  double ms_text_copy;     /* the text, device to host (HIP events) */
  uint64_t bytes_h2d, bytes_d2h, text_bytes, n_pieces;
  double ms_svsig;         /* LRA_PACK_SVSIG: the signatures, their text, its copy to the host (wall); its bytes are in none of the fields above */
  uint64_t svsig_bytes_h2d, svsig_bytes_d2h, svsig_text_bytes;   /* the names up; the text, rec_off and the totals down */
} lra_records_device_stats;
int lra_map_records_device(lra_ctx* ctx, const lra_map_result* res, const lra_map_opts* opts, const char* const* names, const char* const* reads,
                           const char* const* quals, const int32_t* read_len, const char* const* chrom_names, const char* const* passthrough,
                           const char* d_qual, const uint64_t* d_qual_off, int flags, int n_threads, const char** text, uint64_t* len,
                           const uint64_t** rec_off);
int lra_map_records_device_last(lra_ctx* ctx, lra_records_device_stats* out);
/* lra_map_records_device whose record text leaves the device BGZF-compressed (additive to ABI 9): the arguments, the flags, rec_off (in UNCOMPRESSED
 * bytes) and the SV signature text (plain, through lra_map_records_device_svsig) are those of lra_map_records_device.  Formats 's', 'P' and 'a': the
 * text's own device-to-host copy is skipped and lra_bgzf_compress_device runs on the text where the assembly left it; the fall-through formats 'p' and
 * 'b' upload the host text and compress it the same way.  data / data_len / member_off / n_members: as lra_bgzf_compress_device returns them (owned by
 * the context, valid until its next compress call; no EOF member).  lra_map_records_device_last then has the members' bytes in bytes_d2h instead of the
 * text's; lra_bgzf_compress_stats gives the compress stage's wall time (ms_deflate) and its output (bgzf_bytes). */
int lra_map_records_device_bgzf(lra_ctx* ctx, const lra_map_result* res, const lra_map_opts* opts, const char* const* names, const char* const* reads,
                                const char* const* quals, const int32_t* read_len, const char* const* chrom_names, const char* const* passthrough,
                                const char* d_qual, const uint64_t* d_qual_off, int flags, int n_threads, const uint8_t** data, uint64_t* data_len,
                                const uint64_t** rec_off, const uint64_t** member_off, uint64_t* n_members);
int lra_map_records_device_svsig(lra_ctx* ctx, const char** text, uint64_t* len, const uint64_t** rec_off);
/* ---- BAM output (additive to ABI 9) ----------------------------------------------------------------------------------------------------------------
 * lra_map_records_device_bam: the batch's records as BAM alignment records (SAM/BAM specification 4.2: block_size, the 32-byte core, the name, the
 * CIGAR ops, SEQ as 4-bit codes, QUAL as phred bytes, the typed tags), which say what lra_map_records_device's SAM text (printFormat 's') of the same
 * result under the same options says: the same grouping, order, MAPQ, flags and clips, the same hardClip rule, PrintNumAln, MD:Z under LRA_PACK_MD,
 * SA:Z and passthrough tags; unaligned, flagged and handed-back reads follow the same rules.  Arguments and flags are lra_map_records_device's (reads
 * may be NULL).  printFormat other than 's', a read name above 254 bytes and a passthrough text that is not SAM aux fields (TG:T:value, tab-separated)
 * are LRA_ERR_INVALID; the last two name the read.  The split is lra_map_records_device's: the host writes the core, the name, the clip ops, the tag
 * block (integers typed as the smallest of C S I / c s i that holds them, NV:f as the float's bytes, TP:A, MD:Z / SA:Z with a NUL; passthrough text
 * turned into binary aux) as literals of the piece table; the device makes the CIGAR ops, the packed SEQ and the phred QUAL once each
 * (lra_bam_cigar_batch, lra_bam_pack_seq_batch, lra_bam_phred_batch) and the copy pass of lra_map_records_device assembles the records; block_size is
 * written behind it, a lane per record.
 *   core      refID = the chromosome's index, pos = t_start, bin = reg2bin(t_start, t_end), next_refID = next_pos = -1, tlen = the bits of the SAM's
 *             column 9 (t_end - t_start); an unaligned record has refID = pos = -1, bin 4680, flag 4 and no CIGAR.
 *   QUAL      BAM's QUAL has l_seq bytes: where the SAM's QUAL is not as long as its SEQ (hardClip's supplementary records, whose two ranges differ; a
 *             quality string shorter than its read; "*"; no qualities) the record has none (0xff).  A reverse-strand record's qualities stay as they came.
 *   CG:B:I    a record with more CIGAR ops than the limit (65535; lra_bam_set_cigar_limit, 1 .. 65535, 0: the default -- for tests) has the CIGAR
 *             <l_seq>S<t_end - t_start>N and its ops in a CG:B:I tag at the end of the tag block, as the specification says.
 * bgzf = 0: *data[0, *data_len) is the raw record stream in the context's page-locked record buffer, *member_off = NULL, *n_members = 0.  bgzf = 1: the
 * stream stays on the device and goes through lra_bgzf_compress_device; data / data_len / member_off / n_members are as lra_map_records_device_bgzf
 * returns them (no EOF member).  (*rec_off)[n_reads + 1] is per read, in bytes of the uncompressed stream.  The stream is in read order, not coordinate
 * order: no index and no virtual offsets come with it.  LRA_PACK_SVSIG works as in lra_map_records_device (the signature text is plain);
 * lra_map_records_device_last reports this call too.  The file's writer puts lra_bam_header's bytes in front and the BGZF EOF member behind.
 * lra_bam_header (host only, two-call convention): "BAM\1", l_text, the text (lra_format_sam_header's, as it is), n_ref and per reference l_name, the
 * name with its NUL and l_ref = chrom_pos[i + 1] - chrom_pos[i]. */
int lra_map_records_device_bam(lra_ctx* ctx, const lra_map_result* res, const lra_map_opts* opts, const char* const* names, const char* const* quals,
                               const int32_t* read_len, const char* const* chrom_names, const char* const* passthrough, const char* d_qual,
                               const uint64_t* d_qual_off, int flags, int n_threads, int bgzf, const uint8_t** data, uint64_t* data_len,
                               const uint64_t** rec_off, const uint64_t** member_off, uint64_t* n_members);
int lra_bam_set_cigar_limit(lra_ctx* ctx, int ops);
int lra_bam_header(const char* text, uint64_t text_len, int n_chrom, const char* const* chrom_names, const uint64_t* chrom_pos, uint8_t* out, uint64_t cap,
                   uint64_t* len);
/* The device primitives behind it (gfx950; device arrays, on ctx's device and stream, complete at return; results owned by the context and valid until
 * the next call of the same primitive on it; nothing is written behind the last byte or in front of the first).
 *   lra_bam_cigar_batch     arguments as lra_cigar_text_batch.  One lane per run: (len << 4) | {0 1 2 3} for = X I D becomes BAM's (len << 4) | {7 8 1 2};
 *                           a positive clip is an S (clip_op 'H': H) op on its side of the alignment's ops.  d_off[n_aln + 1] is in ops.
 *   lra_bam_pack_seq_batch  range i = d_src[off, off + len) as 4-bit codes, (len + 1) / 2 bytes, the first base in the high nibble, an odd tail's low
 *                           nibble 0; the ranges back to back at d_off[n + 1] (bytes).  "=ACMGRSVTWYHKDBN" in either case are 0 .. 15, any other byte 15.
 *                           A range that leaves d_src[0, src_bytes) is not read: its bases are 15.
 *   lra_bam_phred_batch     request i = len bytes: character - 33 of read's quality string d_qual[d_qual_off[read] + pos ..] where [pos, pos + len) lies
 *                           inside the string; otherwise (d_qual NULL, read >= n_reads, the string too short, empty or "*") every byte is 0xff. */
typedef struct lra_bam_cigar_result { int32_t n_aln; uint64_t n_ops; const uint64_t* d_off; const uint32_t* d_ops; } lra_bam_cigar_result;
typedef struct lra_bam_seq_range { uint64_t off, len; } lra_bam_seq_range;
typedef struct lra_bam_qual_req { uint32_t read, pos, len, reserved; } lra_bam_qual_req;
typedef struct lra_bam_bytes_result { uint64_t n, n_bytes; const uint64_t* d_off; const uint8_t* d_data; } lra_bam_bytes_result;
int lra_bam_cigar_batch(lra_ctx* ctx, int n_aln, const uint32_t* d_runs, const uint64_t* d_run_off, const int32_t* d_pre_clip, const int32_t* d_suf_clip,
                        const uint8_t* d_clip_op, lra_bam_cigar_result* out);
int lra_bam_pack_seq_batch(lra_ctx* ctx, uint64_t n, const lra_bam_seq_range* d_ranges, const uint8_t* d_src, uint64_t src_bytes, lra_bam_bytes_result* out);
int lra_bam_phred_batch(lra_ctx* ctx, uint64_t n, const lra_bam_qual_req* d_req, int n_reads, const char* d_qual, const uint64_t* d_qual_off,
                        lra_bam_bytes_result* out);
/* ---- Coordinate-sorted BAM with a .bai index (additive to ABI 9) -----------------------------------------------------------------------------------
 * lra_bam_sorter holds the raw BAM alignment records of any number of batches in device memory of its own (no work buffer of the context), sorts them
 * on the device and gives them back as BGZF members together with the bytes of the .bai file (SAM specification 5.2).  One sorter serves one context.
 *   create    max_bytes bounds everything the sorter allocates on the device, finish and index included (>= 1; nothing is allocated yet).
 *   add       records d_stream[d_rec_start[i], d_rec_start[i + 1]), i < n_rec: complete records (block_size, core, ...) back to back, device arrays,
 *             copied into an allocation of the batch's own.  LRA_ERR_NOMEM, with nothing changed, when held + the batch + need(held + batch) exceeds
 *             max_bytes: the caller finishes a run and adds again.  More than 2^32 - 1 held records: LRA_ERR_INVALID.  Not between finish and index.
 *   need(N records, B bytes), what finish and index allocate:
 *             the sorted copy of the stream (B + 64) and its record offsets (8 (N + 1)); per sorted record refID, pos, end and bin | unmapped (16 N);
 *             the larger of  the sort's arena -- keys and ordinals twice for rocprim's double buffer (24 N), rocprim's temporary storage, per record
 *             its address and length, and both in sorted order (24 N) --  and  the index's arena -- run heads and their scan (12 N + 8), the run
 *             records and their sort (48 per run, at most N runs, + rocprim's temporary storage), the members' offsets (8 per member), per reference
 *             five counters and (ref_len + 16383) / 16384 + 1 linear-index windows of 8 bytes (known at finish: LRA_ERR_NOMEM there, nothing
 *             changed, if they do not fit) --;  and the compress stage's round (lra_bgzf_compress_device: 2 x 65536 + 32 bytes per member of a
 *             round, lra_bgzf_compress_set_round; these two buffers are the context's and stay with it).
 *   finish    sorts what is held.  Order (samtools sort's default): refID as an unsigned number (-1 last), pos, forward before reverse (flag & 16),
 *             ties in the order added.  One 64-bit key: (refID, -1 as 0x7fffffff) << 33 | (uint32)(pos + 1) << 1 | reverse; rocprim's radix sort runs
 *             over the bits in which the held keys differ.  A record shorter than its core, or a refID >= n_ref: LRA_ERR_INVALID, nothing changed.
 *   next      successive pieces of whole BGZF members (host memory of the context's, valid until the next call): the sorted stream goes through
 *             lra_bgzf_compress_device in slices of (members per round) x LRA_BGZF_IN_MAX bytes, so the members are those of ONE call on the whole
 *             stream.  *len = 0: done.  No EOF member.
 *   index     after the last piece (before: LRA_ERR_INVALID): the .bai bytes (owned by the sorter, valid until its next finish or its destruction).
 *             Afterwards the sorter is empty and takes the next run.  A reference above 2^29 bases: LRA_ERR_INVALID with the reason (BAI cannot
 *             address it; the members were delivered, the sorter is empty; CSI is out of scope).
 * Virtual offsets.  Byte u of the sorted stream is ((first_member_file_offset + member_off[u / 65280]) << 16) | (u % 65280); a record that ends on a cut
 * ends at the next member's start with offset 0, behind the last member that is the EOF member the writer appends.
 * The .bai rules (lra_bam_index_host states them as code; both forms write the same bytes):
 *   - only records with refID >= 0 are indexed, under the bin of their own core field;
 *   - a run is a maximal sequence of consecutive records in file order with the same (refID, bin); each run is one chunk [voff(start of its first
 *     record), voff(end of its last)); a bin's chunks are in file order; nothing is merged further;
 *   - a reference's bins ascend by number; a reference with records also gets the pseudo-bin 37450, last and counted in n_bin, with the two chunks
 *     (voff of its first record, voff end of its last) and (n_mapped, n_unmapped by flag & 4);
 *   - a record's end is pos + max(1, the lengths of its CIGAR ops M D N = X); window w (16384 bases) of the linear index holds the smallest start
 *     offset of a record with pos >> 14 <= w <= (end - 1) >> 14 (a record that reaches past its reference's end counts up to the window of that end);
 *     n_intv = the last touched window + 1; an untouched window takes the value of the next touched one behind it; pos < 0 counts as 0;
 *   - a reference without records has n_bin = n_intv = 0; the trailing n_no_coor counts the records with refID = -1.
 * lra_bam_index_host (host only, two-call convention: out NULL sets *len; cap < *len is LRA_ERR_INVALID): the same bytes from a sorted raw stream and
 * the member table ((n_members + 1) offsets), walked serially.  A record cut short, a refID outside [-1, n_ref) or a reference above 2^29 bases:
 * LRA_ERR_INVALID.
 * lra_map_records_device_bam_to_sorter: lra_map_records_device_bam's encoding, with nothing copied to the host and nothing compressed: the stream and
 * the record starts (the assembly's piece-length scan at every record's first piece) go to the sorter.  rec_off as lra_map_records_device_bam. */
typedef struct lra_bam_sorter lra_bam_sorter;
int lra_bam_sorter_create(lra_ctx* ctx, uint64_t max_bytes, lra_bam_sorter** out);
void lra_bam_sorter_destroy(lra_bam_sorter* s);
int lra_bam_sorter_add_device(lra_bam_sorter* s, const uint8_t* d_stream, const uint64_t* d_rec_start, uint64_t n_rec);
int lra_bam_sorter_held(lra_bam_sorter* s, uint64_t* n_rec, uint64_t* bytes);
int lra_bam_sorter_finish(lra_bam_sorter* s, uint64_t first_member_file_offset, int n_ref, const uint64_t* ref_len);
int lra_bam_sorter_next(lra_bam_sorter* s, const uint8_t** h_data, uint64_t* len);
int lra_bam_sorter_index(lra_bam_sorter* s, const uint8_t** h_bai, uint64_t* len);
/* per stage of the last finish / next / index, HIP events (ms): keys + span, the sort, the gather, the compress stage (wall), the index */
int lra_bam_sorter_stats(lra_bam_sorter* s, double ms[5]);
int lra_bam_index_host(const uint8_t* stream, uint64_t len, int n_ref, const uint64_t* ref_len, const uint64_t* member_off, uint64_t n_members,
                       uint64_t first_member_file_offset, uint8_t* out, uint64_t cap, uint64_t* out_len);
int lra_map_records_device_bam_to_sorter(lra_ctx* ctx, const lra_map_result* res, const lra_map_opts* opts, const char* const* names,
                                         const char* const* quals, const int32_t* read_len, const char* const* chrom_names,
                                         const char* const* passthrough, const char* d_qual, const uint64_t* d_qual_off, int flags, int n_threads,
                                         lra_bam_sorter* sorter, const uint64_t** rec_off);
/* ---- Merging coordinate-sorted BAM files (additive to ABI 9) ---------------------------------------------------------------------------------------
 * lra_bam_merger streams n_runs (1 .. 256) coordinate-sorted BAM files -- each a complete file: header, records that may begin in the middle of a
 * member, an optional EOF member; all with the same reference table -- into one sorted stream, given back as BGZF members with the bytes of the .bai
 * file.  The order is the sorter's key, computed by the sorter's code; ties keep run order, then file order within a run: runs that a sorter made from
 * successive batches merge into the stream one sorter with an unbounded budget gives, member for member and index byte for index byte.
 *   create    sniffs every file and parses its header on the host; a file that is no BAM file, or whose n_ref, names or lengths differ from the first
 *             run's: LRA_ERR_INVALID naming the file and the first difference.  n_runs outside 1 .. 256: LRA_ERR_INVALID (256 runs is the limit; a
 *             merge of merges is not built).  window_bytes: the compressed bytes a run reads per refill, at least 65536 (smaller values are raised to
 *             it) and never more than the file still holds; 0: max_bytes / (24 n_runs), within [65536, 2^28] -- a window, its decoded bytes twice, its
 *             arrays and its share of the round take about twenty times its compressed bytes at BAM's usual ratios.
 *   header    the first run's uncompressed header bytes and the reference lengths (owned by the merger).  The caller writes the header and passes
 *             the length of what it wrote in front of the first member as first_member_file_offset.
 *   next      pieces of whole BGZF members, at most (members per round of the compress stage) x LRA_BGZF_IN_MAX bytes of the stream each; *len = 0:
 *             done.  No EOF member.
 *   index     after the last piece (before: LRA_ERR_INVALID): the .bai bytes, by the sorter's rules.  A reference above 2^29 bases: LRA_ERR_INVALID
 *             with the reason, after the members were delivered.
 * A round.  Every run owns a window: the whole records of its last refill, framed and keyed once.  The bound is the smallest (key of the window's last
 * record, run) over the runs that have bytes behind their window; a run emits its records with (key, run) <= bound, every run everything when no run
 * sets a bound.  The bound's run emits its whole window, so every round makes progress; a record not yet seen is never smaller than an emitted one,
 * and one of the bound's own run that equals the bound sorts behind everything emitted by the tie rule.  A record's place in the round is its ordinal
 * among its run's emitted records + the emitted records of every earlier run with key <= its own + those of every later run with key < its own (a
 * merge by ranks: binary searches, no second sort).  The round is gathered behind what the last round left, its whole multiples of LRA_BGZF_IN_MAX
 * bytes are compressed and the rest waits, so the members are those of ONE lra_bgzf_compress_device call on the merged stream and the sorter's formula
 * for virtual offsets holds.  Only windows a round emptied are refilled; the others keep their records and keys.
 * Refusals (LRA_ERR_INVALID naming the file; the merger then only refuses): keys that descend, with the record's ordinal in its file; a record shorter
 * than its fields or a refID >= n_ref; a bad BGZF member; a file that ends inside a record.
 * Budget.  max_bytes bounds the device memory of the merger (the compress stage's round is the context's, as for the sorter).  With, per run r that
 * still reads, C_r the compressed bytes of its refill, M_r their members, D_r the decoded bytes of its window with the carried tail and N_r its records:
 *     need = sum over r of [ C_r + 1  +  2 (D_r rounded up to 4096 + 64)  +  20 (M_r + 1)  +  8 (D_r / 36 + 2)  +  24 N_r ]          (the windows)
 *          + 80 n_runs + 128  +  (B + 65280 + 64) + 65280  +  72 E + 16                                    (a round of E records, B bytes)
 *          + 8 (5 n_ref + 1) + 8 (n_ref + 1) + 8 (sum((ref_len + 16383) / 16384 + 1) + 1)                  (the index, resident)
 * The step's own buffers (the first three terms of a window) have a floor of 4096 items and are never shrunk; the merger's arrays are allocated an
 * eighth larger than asked and never shrunk.  A run whose file is wholly in its window keeps the decoded bytes, the starts and the keys only, and
 * nothing once its last record is emitted.  The members of a refill are walked on the host before anything is allocated for them, and a refill or a
 * round that would pass max_bytes is LRA_ERR_NOMEM with the figure needed (the merger then holds nothing on the device); a record larger than its
 * window doubles the window's refill under the same check.  At index the window buffers are gone and each reference's chunks are sorted by bin in 24
 * bytes per chunk + rocprim's temporary storage.
 * Index.  Kept in stream-offset space while the rounds run: chunk boundaries as byte offsets u, the linear index's windows as the minimum u (64-bit
 * atomicMin, resident on the device), per reference first / last / counters; a chunk that continues over a round's edge is extended on the host.  The
 * virtual offset is monotone in u, so index converts with the complete member table and writes through the sorter's writer.
 * lra_bam_merger_stats: rounds, records and bytes delivered, refills per run, the peak of the merger's device bytes, ms per stage (read + inflate and
 * compress: wall; the others: HIP events). */
typedef struct lra_bam_merger lra_bam_merger;
struct lra_bam_merger_stats {
  uint64_t rounds, records, bytes, peak_device_bytes;
  uint64_t refills[256];
  double ms_read_inflate, ms_frame_keys, ms_bound_rank, ms_gather_span, ms_compress, ms_index;
};
int lra_bam_merger_create(lra_ctx* ctx, uint64_t max_bytes, uint64_t window_bytes, int n_runs, const char* const* paths,
                          uint64_t first_member_file_offset, lra_bam_merger** out);
int lra_bam_merger_header(lra_bam_merger* m, const uint8_t** h_bytes, uint64_t* len, int* n_ref, const uint64_t** ref_len);
int lra_bam_merger_next(lra_bam_merger* m, const uint8_t** h_data, uint64_t* len);
int lra_bam_merger_index(lra_bam_merger* m, const uint8_t** h_bai, uint64_t* len);
int lra_bam_merger_stats(lra_bam_merger* m, struct lra_bam_merger_stats* out);
void lra_bam_merger_destroy(lra_bam_merger* m);
/* ---- BAM to SAM text, whole or by region through the .bai (additive to ABI 9) -----------------------------------------------------------------------
 * lra_bam_view prints the alignment records of a BAM file -- this project's or any other's -- as SAM lines on the device: the inverse of the BAM
 * encoder and the reader of the index the sorter and the merger write.  One view serves one context and owns its device memory (no work buffer).
 *   create    sniffs the file (not BAM: LRA_ERR_INVALID), inflates and parses the header on the host.  bai_path (NULL: none) is read and checked whole:
 *             every count and length against the bytes that remain; a negative n_bin / n_chunk / n_intv, a chunk with end < beg, an n_ref other than
 *             the BAM header's, bytes behind n_no_coor: LRA_ERR_INVALID with the reason.  The pseudo-bin 37450 is no bin; n_no_coor may be absent.
 *             window_bytes: the compressed bytes a step reads, at least 65536 (smaller values are raised); 0: 16 MiB.
 *   header    the header text (not NUL-terminated), the reference names and lengths; owned by the view.
 *   set_flags a record is kept if (flag & require) == require && (flag & exclude) == 0; holds for the passes started afterwards and the one running.
 *   all       starts a pass over every record of the file, from the first one behind the header, in windows.
 *   region    starts a pass over the records that overlap [beg, end) of reference ref_id (0-based, half-open; end is clamped to the reference's
 *             length): refID == ref_id && pos < end && pos + max(1, span) > beg, span = the reference bases of the core CIGAR (the index's rule; the N
 *             op of the CG:B:I form carries it).  Without an index, ref_id outside [0, n_ref) or beg > end: LRA_ERR_INVALID.  Either call may be
 *             repeated on one view; each starts a new pass.
 *   next      the next piece: whole SAM lines, each ending in '\n', in file order, each record once; page-locked memory of the view, valid until the
 *             next call on it.  *len = 0: the pass is over.  *n_records (optional): the lines of the piece.
 *   stats     windows, records, bytes read / inflated / printed, ms per stage (read + inflate: wall, one figure -- the step reads and inflates in one
 *             call --; frame + select, tags + lengths, the floats' round trip, emit, the copy to the host: HIP events), summed over the view's life.
 * The plan of a region (lra_bai_query_host states it as code, on the host, without a GPU: index bytes in, chunks out as (beg, end) pairs of virtual
 * offsets, owned by the library and valid until the calling thread's next call): the chunks of reg2bins(beg, end)'s bins; min_off = lin[beg >> 14] (a
 * window behind the last one: no record reaches beg, the plan is empty); each chunk's start raised to min_off, a chunk this empties dropped; sorted by
 * start, chunks that overlap or touch merged: ascending, disjoint, no record read twice.  beg == end gives an empty plan.  n_ref < 0: not compared.
 * A chunk [vb, ve) is read from file offset vb >> 16 with a fresh BGZF step, framed from decoded offset vb & 0xffff; records that start in front of ve are
 * taken (the step's member table maps ve to a decoded position).  At the first record with refID > ref_id, or refID == ref_id && pos >= end, the chunk is
 * over: the file is sorted (the view does not verify it).  A record larger than the window makes the step read on with twice the window.  Planned
 * chunks that lie less than window_bytes apart in the file are read as one chunk from the first's start to the last's end: the records between them
 * are in file order too and fail the overlap test, and a step per chunk costs a member's inflate latency (about 10 ms) each.
 * The text.  QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL and the tags in the file's order, tab-separated.  RNAME '*' for refID < 0; POS and
 * PNEXT the stored value + 1; CIGAR '*' with 0 ops; a core CIGAR <l_seq>S<n>N with a CG:B:I tag prints the tag's ops and not the tag; RNEXT '*' for
 * next_refID < 0 (or outside the table), '=' when it equals refID, else the name; SEQ '*' for l_seq = 0, else through "=ACMGRSVTWYHKDBN"; QUAL '*' for
 * l_seq = 0 or a first byte of 0xff, else + 33.  Tags: c C s S i I print as TAG:i:value; A, Z, H their bytes; B as B:<subtype> and ,value per element;
 * f (and the elements of B:f) as printf("%.6g", (double)v) -- printed on the host: one array of floats out, their text back, per window.
 * Refusals (LRA_ERR_INVALID naming the file and the record's ordinal -- in a region pass its ordinal among the records read from a compressed
 * offset --; the records in front of the fault are delivered first, the next call refuses, and the view takes another pass): a BGZF fault (the
 * readers' text); a block_size below 32; a record with l_read_name = 0, no NUL behind its name, 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 +
 * l_seq > block_size or a refID outside [-1, n_ref); a CIGAR op code above 8; an aux block that ends inside a tag or names a type outside
 * A c C s S i I f Z H B (B: c C s S i I f); a file that ends inside a record.
 * Memory.  With C = the compressed bytes of a window (window_bytes, or more for a larger record), M its members, D its decoded bytes with the carried
 * tail, N its framed records, T their printed tags, E their array elements and single floats, F the floats among them, O their CIGAR ops and X the
 * bytes of their text, a window allocates on the device
 *     C + 1 + 2 (D rounded up to 4096 + 64) + 20 (M + 1)                                        (the step; C + 1 more page-locked on the host)
 *   + 8 (D / 36 + 2) + 92 N (region passes: + 16 N) + 40 T + 12 E + 12 O + 20 F + the floats' text + 22 (7 N + T) + X + 64
 * each array an eighth larger than asked and never shrunk; X + 1 bytes of page-locked host memory take the text. */
typedef struct lra_bam_view lra_bam_view;
struct lra_bam_view_stats {
  uint64_t windows, records, bytes_read, bytes_inflated, bytes_text;
  double ms_read_inflate, ms_frame_select, ms_tags_lengths, ms_floats, ms_emit, ms_copy;
};
int lra_bam_view_create(lra_ctx* ctx, const char* bam_path, const char* bai_path, uint64_t window_bytes, lra_bam_view** out);
int lra_bam_view_header(lra_bam_view* v, const char** text, uint64_t* text_len, int* n_ref, const char* const** names, const uint64_t** ref_len);
int lra_bam_view_set_flags(lra_bam_view* v, uint32_t require, uint32_t exclude);
int lra_bam_view_all(lra_bam_view* v);
int lra_bam_view_region(lra_bam_view* v, int32_t ref_id, int64_t beg, int64_t end);
int lra_bam_view_next(lra_bam_view* v, const char** h_text, uint64_t* len, uint64_t* n_records);
int lra_bam_view_stats(lra_bam_view* v, struct lra_bam_view_stats* out);
void lra_bam_view_destroy(lra_bam_view* v);
int lra_bai_query_host(const uint8_t* bai, uint64_t bai_len, int n_ref, int32_t ref_id, int64_t beg, int64_t end, const uint64_t** chunks,
                       uint64_t* n_chunks);
/* ---- BAM depth: per-base and binned coverage, whole or by region through the .bai (additive to ABI 9) ----------------------------------------------
 * lra_bam_depth turns the records of a coordinate-sorted BAM file into coverage on the device.  It reads the file as lra_bam_view does -- the same
 * windows, the same plan and chunk rules for a region, the same refusals (bam_pass.h is the one code of both) -- and owns its device memory; one
 * object serves one context.  A pass covers the whole file (all) or [beg, end) of one reference (region: lra_bam_view_region's conventions -- 0-based,
 * half-open, end clamped to the reference's length, beg == end an empty pass, no index or a bad ref_id LRA_ERR_INVALID).
 * Which records count.  refID >= 0, (flag & require) == require && (flag & exclude) == 0 (exclude ~0u: 0x704 -- unmapped, secondary, QC fail,
 * duplicate) and mapq >= min_mapq.
 * How ops count.  The core CIGAR's ops; those of the CG:B:I tag when the core CIGAR is <l_seq>S<n>N and the record has the tag (wherever it stands in
 * the aux block).  M = X add 1 to every reference position they cover; D advances and adds only with count_deletions; N advances and never adds;
 * I S H P neither advance nor add; a record of 0 ops adds nothing.  Depth is uint32.  Positions outside the reference (or the region) are dropped.
 * Per-base text (bin == 0): RNAME \t POS (1-based) \t DEPTH \n for the positions with depth > 0; all_positions: for every position of the pass's range,
 * in a whole-file pass every position of every reference in header order.
 * Binned text (bin > 0): RNAME \t START (0-based) \t END \t MEAN \n for every bin [b0 + k bin, min(b0 + (k + 1) bin, range end)), b0 = the pass's beg
 * (0 for whole references), empty bins too.  MEAN in integers: h = (100 sum + len / 2) / len in 64 bits, printed as h / 100 '.' and two digits of h % 100.
 * Values (want_values): uint32 depth[count] per position from `first` on (bin == 0; without all_positions stretches no record reaches are left out
 * and `first` jumps), or uint64 sum[count] per bin from the bin that starts at `first` on (bin > 0).  want_text and want_values may both be set; one
 * of them must be.
 * Pieces come in reference order, then position order.  A delivered piece is final: nothing delivered later changes it, no position or bin comes
 * twice.  A piece's memory is page-locked, owned by the object and valid until the next call on it; count == 0 && text_len == 0: the pass is over.
 * (count is set with or without want_values; a piece may have count > 0 and no text.)
 * Refusals (LRA_ERR_INVALID, the view's texts under this object's name): a BGZF fault, a block_size below 32, a record the view's arithmetic
 * refuses, a refID outside [-1, n_ref), a CIGAR op code above 8, an aux block that ends inside a tag while the CG tag of a counted <l_seq>S<n>N record
 * is looked for, a file that ends inside a record -- and a record whose (refID, pos), refID -1 last, sorts in front of its predecessor's, across
 * window edges too: "not coordinate-sorted at record N".  The pieces the records in front of the fault made final are delivered first, the next call
 * refuses, and the object takes another pass.
 * Memory.  The position window: int32 diff[span_bases + 2], twice, holds [base, base + span) of the current reference; positions below the next
 * window's first record are final, finished (scanned, delivered) and the base slides; a window whose records reach beyond it is taken in prefixes,
 * and a single record longer than it doubles span_bases.  window_bytes as the view's; span_bases 0: 4 Mi positions, below 65536: raised.
 * Stats, summed over the object's life: windows, records read / counted / filtered, slides, positions with depth > 0, the sum and the maximum of the
 * depth delivered (a pass adds these three when it is over), bytes read / inflated / delivered, ms per stage (read + inflate: wall; the rest HIP
 * events). */
typedef struct lra_bam_depth lra_bam_depth;
struct lra_bam_depth_opts {
  uint32_t require, exclude, min_mapq, count_deletions, bin, all_positions, want_text, want_values;
  uint64_t window_bytes, span_bases;
};
struct lra_bam_depth_piece {
  int32_t ref_id; int64_t first; uint64_t count;
  const uint32_t* depth; const uint64_t* sum; const char* text; uint64_t text_len;
};
struct lra_bam_depth_stats {
  uint64_t windows, records_read, records_counted, records_filtered, slides, covered, depth_sum, depth_max, bytes_read, bytes_inflated, bytes_delivered;
  double ms_read_inflate, ms_frame_select, ms_ops, ms_accumulate, ms_finish, ms_text, ms_copy;
};
int lra_bam_depth_create(lra_ctx* ctx, const char* bam_path, const char* bai_path, const struct lra_bam_depth_opts* opts, lra_bam_depth** out);
int lra_bam_depth_header(lra_bam_depth* d, int* n_ref, const char* const** names, const uint64_t** ref_len);
int lra_bam_depth_all(lra_bam_depth* d);
int lra_bam_depth_region(lra_bam_depth* d, int32_t ref_id, int64_t beg, int64_t end);
int lra_bam_depth_next(lra_bam_depth* d, struct lra_bam_depth_piece* piece);
int lra_bam_depth_stats(lra_bam_depth* d, struct lra_bam_depth_stats* out);
void lra_bam_depth_destroy(lra_bam_depth* d);
/* ---- BAM to VCF: the insertions and deletions of every alignment, whole or by region through the .bai (additive to ABI 9) ---------------------------
 * lra_bam_vcf prints one VCF line per insertion and deletion of the alignments of a BAM file, on the device: the step behind the aligner in the
 * reference's "call SVs from lra alignments" pipeline (call_assembly_SVs/SamToVCF.py).  It reads the file as lra_bam_view and lra_bam_depth do -- the
 * same windows, the same plan and chunk rules for a region, the same refusals (bam_pass.h is the one code of the three) -- and owns its device memory;
 * one object serves one context.  No base of SEQ is compared with the genome: mismatches are not variants (the script never prints one).
 *   create    the context must hold a genome and a chromosome table (lra_ctx_load_genome[_device], lra_ctx_load_chromosomes; upper case, as the
 *             script's ref.fetch(...).upper()).  n_chrom == n_ref and every chromosome's length against the BAM header's: no genome, or any
 *             difference, is LRA_ERR_INVALID naming the first reference that differs.  Chromosomes are matched to references by index, not by name:
 *             the context holds no names.  The test is repeated when a pass starts and at every next.
 *   opts      require / exclude as lra_bam_depth's; exclude ~0u means 0x4 (pysam's fetch yields every mapped record, secondary and supplementary
 *             included).  min_mapq.  min_length: a variant is kept if |len(ALT) - len(REF)| >= min_length; 0 is raised to 1.  pos_one_based 0: POS is
 *             the 0-based position of the anchor base, as the script prints it; 1: that + 1, as VCF means it.  want_text, want_values (one of them
 *             must be set), window_bytes as the view's.  drop_contained (the field that was `reserved`; 0: off, today's output): see below.  NULL
 *             opts: the defaults, text only.
 * drop_contained: the reference's ParseAlignment.py, the step in front of SamToVCF.py in call_assembly_SVs, which drops every alignment that lies inside
 * an earlier one so that a nested contig alignment does not call the same indel again.  The filter runs over the records with refID >= 0 in file order,
 * in front of the flag and MAPQ filters (the script sees every line).  e(i) = pos + 1 + tlen in 64 bits, tlen the stored field (lra writes
 * tEnd - tStart: Alignment.h says the script depends on it; the field may be negative).  The first record of each run of equal refID is kept; record i
 * is dropped when e(i) <= the largest e(j) of the earlier records j of its run -- equal ends drop.  (The script compares with the end of the last kept
 * record, which is that maximum: a dropped record never exceeds it.)  On the device: a segmented max-scan over the window's records
 * (bam_contained.h), the last refID and its running maximum carried from window to window and moved on only when a window is delivered, so a window
 * run again in front of a refused record starts from the same carry.  It holds for a pass over the whole file and for a region pass with beg == 0,
 * which reads every record of the reference with pos < end in order; lra_bam_vcf_region with beg > 0 and the filter on is LRA_ERR_INVALID and says
 * why.  Dropped records are not walked, count in records_contained and not in records_filtered; `record` still counts every record read.  The filter
 * adds 4 N + 24 (N / 2048 + 3) device bytes to a window of N records.
 * Which records are walked.  refID >= 0, (flag & require) == require && (flag & exclude) == 0, mapq >= min_mapq, at least one op, l_seq > 0 and at
 * least one M = X base.  The ops are the core CIGAR's, or those of the CG:B:I tag when the core CIGAR is <l_seq>S<n>N and the record has the tag
 * (lra_bam_depth's rule and code).  A record that passes the filters and has no op, l_seq = 0 or no M = X base is skipped and counted (the script
 * raises IndexError / TypeError on these); the others that are not walked count as filtered.
 * The walk, over the ops in order with two counters, q in SEQ (from 0) and r on the reference (from pos).  Ops of length 0 and H and P yield nothing
 * and do not part a run.  M = X advance both; aq = q - 1 behind them is the SEQ index of the last aligned base.  Everything in front of the first M = X
 * base is skipped (it only advances the counters).  Behind it, consecutive I / S ops form one insertion run (they advance q) and consecutive D / N ops
 * one deletion run (they advance r): I P I and I I are one run, D N D is one run.  With r0 the value of r where the run begins, its anchor is the
 * reference base r0 - 1: the last base in front of the run, aligned or -- behind a deletion run -- deleted.  aq does not move in either run.  A run that
 * is followed by another entry (an M = X base or a run of the other kind) is a variant; a run that reaches the end of the CIGAR is none.
 *   INS   POS = r0 - 1, REF = the genome base there, ALT = SEQ[aq, q) with q behind the run: from the anchor through the last inserted base
 *   DEL   POS = r0 - 1, REF = the genome [r0 - 1, r) with r behind the run: from the anchor through the last deleted base, ALT = SEQ[aq]
 * QSTART = aq + 1.  REF's first base comes from the genome and ALT's first from the read: they differ when the anchor is a mismatch.  SEQ is decoded
 * through "=ACMGRSVTWYHKDBN"; genome bytes are copied as loaded, from chrom_pos[refID] + position.  SVLEN = len(ALT) - len(REF); SVTYPE is DEL if it is
 * negative, else INS.
 * Where the script is not followed.  (1) An insertion run directly followed by a deletion run: the script takes the rest of the read as ALT; here ALT
 * ends with the run's last inserted base, which is the script's rule wherever the next entry has a query position.  (2) The records the script would
 * crash on (above) are skipped and counted.  (3) Chromosomes are matched to the genome by index, not by name.
 * The line:  RNAME \t POS \t . \t REF \t ALT \t 60 \t PASS \t SVTYPE=%s;SVLEN=%d;QNAME=%s;QSTART=%d;QSTRAND=%c \t GT \t 1/1 \n, QSTRAND '-' for flag
 * 0x10.  Lines come in the file's order of the records and within a record in CIGAR order; nothing is sorted.
 * Region (lra_bam_view_region's conventions: 0-based, half-open, end clamped, beg == end an empty pass, no index or a bad ref_id LRA_ERR_INVALID): the
 * pass reads the records that overlap [beg, end) and prints the variants whose anchor position, 0-based, lies in [beg, end).  Over a whole reference
 * this is the script's --chrom.
 * Values (want_values): one lra_bam_vcf_variant per line, in the lines' order: ref_id, the anchor's 0-based position (whatever pos_one_based says),
 * qstart, svlen, kind (0 INS, 1 DEL), strand (1 for flag 0x10), record = the record's 0-based ordinal among the records the pass has read (in a pass
 * over the whole file: in the file), text_off = where its line begins in the piece's text (0 without text).
 * Pieces: whole lines, one piece per window that has variants, in page-locked memory of the object, valid until the next call on it; n_variants == 0
 * && text_len == 0: the pass is over.
 * Refusals (LRA_ERR_INVALID, the pass's own under this object's name -- a BGZF fault, a bad block_size or record, an aux block that ends inside a tag
 * while a CG tag is looked for, a file that ends inside a record -- and): a record that passes the filters with an op code above 8; a walked record
 * whose query-consuming ops (M I S = X) do not sum to l_seq; a walked record with pos < 0 or whose reference span ends beyond its reference.  The
 * lowest record of a window is refused, for the first of these reasons that holds.  The records in front of the fault are delivered first, the next
 * call refuses, and the object takes another pass.
 * Memory.  Beside the step's and the frame's arrays (lra_bam_view's formula: C + 1 + 2 (D + 4096 + 64) + 20 (M + 1) + 8 (D / 36 + 2)), a window of N
 * framed records with O ops in G runs and V variants whose lines take X bytes allocates on the device
 *     32 N (region passes: + 16 N) + 42 O + 40 G + 176 V + X + 64
 * each array an eighth larger than asked and never shrunk; X + 1 + 40 V bytes of page-locked host memory take the text and the values.  X has no
 * bound a priori -- a deletion's REF is as long as the deletion --: it is the total of the scanned line lengths, in 64 bits, and a text that cannot
 * be allocated is LRA_ERR_NOMEM, never a cut line.
 * Stats, summed over the object's life: windows, records read / walked / filtered / skipped, INS and DEL lines, bytes read / inflated / printed, ms
 * per stage (read + inflate: wall; frame + select, ops, walk, lengths, emit, copy: HIP events). */
typedef struct lra_bam_vcf lra_bam_vcf;
struct lra_bam_vcf_opts {
  uint32_t require, exclude, min_mapq, min_length, pos_one_based, want_text, want_values, drop_contained;
  uint64_t window_bytes;
};
struct lra_bam_vcf_variant {
  uint64_t record, text_off; int64_t svlen;
  int32_t ref_id, pos; uint32_t qstart; uint8_t kind, strand; uint16_t pad;
};
struct lra_bam_vcf_piece {
  uint64_t n_variants; const struct lra_bam_vcf_variant* variants; const char* text; uint64_t text_len;
};
struct lra_bam_vcf_stats {
  uint64_t windows, records_read, records_walked, records_filtered, records_skipped, n_ins, n_del, bytes_read, bytes_inflated, bytes_text;
  double ms_read_inflate, ms_frame_select, ms_ops, ms_walk, ms_lengths, ms_emit, ms_copy;
  uint64_t records_contained;                                  /* appended: what drop_contained dropped */
};
int lra_bam_vcf_create(lra_ctx* ctx, const char* bam_path, const char* bai_path, const struct lra_bam_vcf_opts* opts, lra_bam_vcf** out);
int lra_bam_vcf_header(lra_bam_vcf* d, int* n_ref, const char* const** names, const uint64_t** ref_len);
int lra_bam_vcf_all(lra_bam_vcf* d);
int lra_bam_vcf_region(lra_bam_vcf* d, int32_t ref_id, int64_t beg, int64_t end);
int lra_bam_vcf_next(lra_bam_vcf* d, struct lra_bam_vcf_piece* piece);
int lra_bam_vcf_stats(lra_bam_vcf* d, struct lra_bam_vcf_stats* out);
void lra_bam_vcf_destroy(lra_bam_vcf* d);
/* ---- Assembly SV calls from a coordinate-sorted BAM: filter, call, size, mask, number, merge (additive to ABI 9) ---------------------------------------
 * lra_bam_svcalls is the one-haplotype half of the reference's call_assembly_SVs/callassemblysv.snakefile on the device: the rules parseAlignment
 * (ParseAlignment.py), CallSV (SamToVCF.py), FilterBySizeAndSVTYPE, FilterByCentromereAndAltChromAndAddID and mergeCalls (bedtools, awk, mergeSV.py).
 * Input is a coordinate-sorted BAM of one haplotype's contig alignments, output the merged DEL and INS tables; the variant table stays on the device
 * from the records to the printed lines.  Combining two haplotypes (Homcalls, Hetcalls, combineHet) is lra_sv_combine's, below.  It is the fourth consumer of the pass
 * (bam_pass.h), and shares the contained filter and the walk with lra_bam_vcf (bam_contained.h, bam_vcf_walk.h); one object serves one context.
 *   create    as lra_bam_vcf_create: the context must hold the genome and its chromosome table, compared with the BAM header's reference table.
 *   opts      require / exclude / min_mapq / window_bytes as lra_bam_vcf's.  drop_contained: lra_bam_vcf's filter (NULL opts: 1).  min_size: a
 *             candidate needs |SVLEN| >= min_size; 0 is raised to 1 (NULL opts: 40).  aligner, hap: the ID's words, printable and without blanks; NULL:
 *             "aligner" and "maternal".  pos_one_based: the text's START and END are printed + 1 (the values never).  vcf_columns: the line has no END
 *             column -- ten columns with the ID third, as a VCF line.  want_text, want_values: one of them must be set (NULL opts: text only).
 * A pass covers the whole file (lra_bam_svcalls_all) or a whole reference (lra_bam_svcalls_region with beg == 0 and end >= the reference's length; it
 * needs the index): anything narrower is LRA_ERR_INVALID, because the merge and the numbering need every row.
 * Per reference, in file order:
 *   candidates  the variants of lra_bam_vcf's walk over the records the contained filter kept, with |SVLEN| >= min_size; the kind is SVLEN's sign.  A row
 *               is START = the anchor's 0-based position (the POS the script prints), END = START + |SVLEN|: FilterBySizeAndSVTYPE's awk, where
 *               len(REF) - len(ALT) = |SVLEN| for a DEL and the converse for an INS.  DEL and INS rows are two independent tables from here on.
 *   mask        lra_bam_svcalls_set_mask(n, ref_id[], beg[], end[]): half-open 0-based intervals in any order, overlapping or not; n = 0 is no mask
 *               (the state after create).  A row is dropped when START < m.end && m.beg < END for an interval m of its reference: bedtools
 *               intersect -v -- one shared base drops, touching does not.  An interval with ref_id outside the header's table, beg < 0 or end < beg is
 *               LRA_ERR_INVALID.  The call ends a pass in hand.  The snakefile's alt-chromosome awk, $1!~/^GL/ || $1!~/^hs37d5/ || $1!~/^NC/, is
 *               always true (no name begins with all three): it drops nothing, and neither is anything dropped here.
 *   numbering   NR counts the rows of a kind that survive the mask from 1, over the pass, in row order: the file's order of the records, then CIGAR
 *               order.  The ID is <aligner>.<DEL|INS>.<hap>.<NR>.  (The snakefile passes -v aln=aligner to awk, so the files it writes carry the
 *               literal word "aligner", not "lra": the default here.)
 *   merge       for rows i, j of one kind and one reference, ov = min(END) - max(START); R(i, j) holds when ov > 0 && 10 ov >= len_i && 10 ov > len_j
 *               with len = END - START: mergeCalls' awk over bedtools intersect -wao, $23 / ($3 - $2) >= 0.1 && $23 / ($14 - $13) > 0.1 (the asymmetry
 *               is the snakefile's; the integer form is the double test exactly: a quotient that is not 1 / 10 differs from it by at least
 *               1 / (10 len), far above an ulp).  In NR order row i is kept unless an earlier KEPT row k has R(k, i): mergeSV.py.  A dropped row
 *               spreads nothing: of A ~ B ~ C with A and C unrelated, A and C are kept.  NR order is not position order (a long record's late
 *               variant precedes the next record's early one).  On the device: every row's earlier related rows as an edge list, then rounds -- a
 *               row is kept once all of them are dropped, dropped once one is kept -- until a round decides nothing; no cap, the result is the serial
 *               walk's for every input.  The pairs are found among the earlier rows of the reference and kind, by tiles of 256 rows in NR order: a tile
 *               whose rows' interval shares no base with the row is passed over, which in a sorted file leaves the tiles near the row.
 *   delivery    a reference's rows are final when a record of a later reference has been delivered or the pass ends.  They come as its DEL piece, then
 *               its INS piece (piece.kind 1, 0; piece.ref_id); a kind without rows has no piece.  One line per kept row, in NR order:
 *                 RNAME \t START \t END \t ID \t REF \t ALT \t 60 \t PASS \t INFO \t GT \t 1/1 \n
 *               REF, ALT and INFO byte for byte lra_bam_vcf's.  Between windows the table keeps, beside its numbers, only what cannot be had again: QNAME
 *               and ALT; REF is read from the resident genome when the line is printed, and only kept rows are printed.
 * Values (want_values): one lra_bam_svcalls_row per kept row: ref_id, start, end (0-based), nr, svlen, qstart, kind (0 INS, 1 DEL), strand, record (the
 * record's ordinal among the records the pass has read), text_off.
 * Pieces live in page-locked memory of the object, valid until the next call on it; n_rows == 0 && text_len == 0: the pass is over.
 * Refusals (LRA_ERR_INVALID): lra_bam_vcf's, under this object's name, and a record that sorts in front of its predecessor by (refID, pos), refID -1
 * last ("the file is not coordinate-sorted at record N"): the filter and the delivery by reference rely on the order.  The pieces of the references
 * that were final in front of the fault -- those with a later reference's record delivered -- come first, then the call refuses; what the unfinished
 * reference had gathered is dropped, and the object takes another pass.
 * Memory.  Beside the step's and the walk's arrays (lra_bam_vcf's formula, the text apart: 32 N (+ 16 N) + 42 O + 40 G + 88 V, + 4 N + 24 (N / 2048 + 3)
 * with the filter), a window with V candidates allocates 24 V + 32; the tables hold 88 bytes per row plus its QNAME and ALT, for the reference in hand
 * and what a window has read of the next, twice at most while rows move to the front; a reference's M rows of a kind with E related pairs and K kept
 * rows whose lines take X bytes allocate 36 M + 16 (M / 256 + 1) + 4 E + 32 K + X + 64 K (values) + 64, each array an eighth larger than asked and never shrunk; X + 1 +
 * 64 K bytes of page-locked host memory take a piece.
 * Stats, summed over the object's life: windows, records read / contained / walked; rows too small, masked, merged away and kept, each for INS and DEL;
 * the merge's deciding rounds; bytes read / inflated / printed; ms per stage (read + inflate: wall; frame + select, ops, walk, lengths -- the walk's --
 * rows, merge, emit, copy: HIP events). */
typedef struct lra_bam_svcalls lra_bam_svcalls;
struct lra_bam_svcalls_opts {
  uint32_t require, exclude, min_mapq, min_size, drop_contained, pos_one_based, vcf_columns, want_text, want_values, reserved;
  uint64_t window_bytes;
  const char* aligner; const char* hap;
};
struct lra_bam_svcalls_row {
  uint64_t record, text_off, nr; int64_t start, end, svlen;
  int32_t ref_id; uint32_t qstart; uint8_t kind, strand; uint16_t pad; uint32_t pad2;
};
struct lra_bam_svcalls_piece {
  uint64_t n_rows; const struct lra_bam_svcalls_row* rows; const char* text; uint64_t text_len; int32_t ref_id; uint32_t kind;
};
struct lra_bam_svcalls_stats {
  uint64_t windows, records_read, records_contained, records_walked, small_ins, small_del, masked_ins, masked_del, merged_ins, merged_del, kept_ins, kept_del,
           merge_rounds, bytes_read, bytes_inflated, bytes_text;
  double ms_read_inflate, ms_frame_select, ms_ops, ms_walk, ms_lengths, ms_rows, ms_merge, ms_emit, ms_copy;
};
int lra_bam_svcalls_create(lra_ctx* ctx, const char* bam_path, const char* bai_path, const struct lra_bam_svcalls_opts* opts, lra_bam_svcalls** out);
int lra_bam_svcalls_header(lra_bam_svcalls* d, int* n_ref, const char* const** names, const uint64_t** ref_len);
int lra_bam_svcalls_set_mask(lra_bam_svcalls* d, uint64_t n, const int32_t* ref_id, const int64_t* beg, const int64_t* end);
int lra_bam_svcalls_all(lra_bam_svcalls* d);
int lra_bam_svcalls_region(lra_bam_svcalls* d, int32_t ref_id, int64_t beg, int64_t end);
int lra_bam_svcalls_next(lra_bam_svcalls* d, struct lra_bam_svcalls_piece* piece);
int lra_bam_svcalls_stats(lra_bam_svcalls* d, struct lra_bam_svcalls_stats* out);
void lra_bam_svcalls_destroy(lra_bam_svcalls* d);
/* ---- Two haplotypes' assembly SV calls as hom / het VCF lines (additive to ABI 9) -----------------------------------------------------------------------
 * lra_sv_combine is the two-haplotype half of call_assembly_SVs/callassemblysv.snakefile on the device: the rules Homcalls, Hetcalls and combineHet.  It
 * owns two lra_bam_svcalls passes -- the maternal BAM's, then the paternal one's, hap words "maternal" and "paternal" -- whose kept rows stay on the device
 * (an internal sink of the pass; such a pass builds no text), classifies every row against the other haplotype's table and prints the six classes.
 *   create    both files as lra_bam_svcalls_create takes one.  The two headers' reference tables must equal the context's (the passes' own test) and each
 *             other, name by name: LRA_ERR_INVALID naming the first difference otherwise.
 *   opts      require / exclude / min_mapq / min_size / drop_contained / window_bytes / aligner / pos_one_based / want_text / want_values as
 *             lra_bam_svcalls'.  frac_num / frac_den: the fraction F of the partner test; 0 / 0 is 3 / 10; den == 0, num == 0 or num > den is
 *             LRA_ERR_INVALID.  filter_pass: the line's FILTER column (below).  NULL opts: the defaults, text only.
 *   inputs    for each kind K in {INS, DEL}: M_K and P_K, the maternal and the paternal pass's kept rows after its own merge, in delivery order (by
 *             reference, then NR), each row with the NR and ID its own pass gave it (<aligner>.<K>.maternal.<NR>, <aligner>.<K>.paternal.<NR>).
 *   partner   rows a, b of one kind and one reference, ov = min(a.end, b.end) - max(a.start, b.start): ov > 0 && den ov >= num (a.end - a.start) &&
 *             den ov >= num (b.end - b.start), in 64 bits.  This is bedtools intersect -f F -r over the .merge.vcf files, whose columns 2 and 3 (START,
 *             END) bedtools reads as BED, half-open -- the reading mergeCalls already relies on.  Symmetric; touching rows are no partners; INS and DEL
 *             rows never meet.  bedtools makes the test in single precision, (float)ov / (float)len >= 0.3f (its source as remembered: bedtools is not
 *             run anywhere here).  For len <= 2^24 = 16777216 the integer form is that test exactly, for 3 / 10 and for 1 / 10: both operands are exact
 *             floats, the quotient is correctly rounded, 0.3f lies above 3 / 10 so equality and everything above it pass, and a quotient below 3 / 10
 *             is below by at least 1 / (10 len), more than the 0.1 * 2^-25 between 3 / 10 and the midpoint under 0.3f (0.3 * 2^-27 for 0.1f).
 *             bam_svcombine_host.h has the numbers, tools/micro/bam_svcombine_host_check.cpp checks them.
 *   classes   hom_K: the rows of M_K with a partner in P_K, each once however many partners it has (-u), with its maternal ID.  het_m_K: the rows of M_K
 *             without one; het_p_K: the rows of P_K without a partner in M_K (-v, both ways round).  A paternal row with a partner is printed nowhere.
 *             Every class keeps its table's order.
 *   line      RNAME \t START \t ID \t REF \t ALT \t 60 \t INFO \t INFO \t GT \t 1/1 \n -- the snakefile's awk prints $9,$9: the FILTER column carries
 *             INFO a second time, and the genotype stays 1/1 in the het files too; what the reference prints is printed.  filter_pass: 60 \t PASS \t
 *             INFO, combinehapSV.snakefile's line (with frac 1 / 10 its whole rule), byte for byte lra_bam_svcalls' line with vcf_columns.  START is
 *             printed + 1 with pos_one_based.
 *   delivery  lra_sv_combine_all / _region (a whole reference only, as lra_bam_svcalls_region) start a run; the first lra_sv_combine_next makes both
 *             passes to their ends -- a row's class needs both tables, and the order is by class, not by reference, so nothing is delivered before --
 *             and then the pieces come in combineHet's order: maternal INS het, maternal DEL het, paternal INS het, paternal DEL het, INS hom, DEL hom
 *             (piece.hap 0 maternal / 1 paternal, kind 0 INS / 1 DEL, cls 0 het / 1 hom; a hom piece has hap 0).  A class without rows has no piece;
 *             n_rows == 0 && text_len == 0: the run is over.  The snakefile cats the SAM header in front of lra.vcf; that slip is not reproduced.
 *   mask      lra_sv_combine_set_mask goes to both passes and ends a run in hand.
 * Values (want_values): one lra_sv_combine_row per printed row: lra_bam_svcalls_row's fields, hap and cls (in that struct's pad bytes).
 * Refusals: a refusal of either pass (lra_bam_svcalls': an unsorted file, a bad record) refuses the lra_sv_combine_next that met it, with that pass's
 * message behind "the maternal pass: " / "the paternal pass: "; nothing is delivered, and the object takes another run.
 * On the device: per pairing (A, B) of M_K against P_K and P_K against M_K, B's rows of a reference are one contiguous range, found by binary search on
 * ref and tiled by 256 rows with each tile's [lowest START, highest END); a lane per row of A passes over the tiles it shares no base with and tests the
 * rows of the others.  B is in NR order, not START order, so there is no early exit on START.  The flag is a function of the two tables alone.
 * Memory.  Beside the two passes' own (lra_bam_svcalls' formula, no text), both haplotypes' kept rows live until the next run: 88 bytes per kept row
 * plus its QNAME and ALT, half as much again while a table grows; 4 bytes per row for the flags; 12 (n_ref + 2) + 16 (K / 256 + n_ref + 1) for a
 * pairing against K rows; a class of C rows out of a table of M whose lines take X bytes allocates 16 M + 32 C + X + 64 C (values) + 64, and X + 1 + 64 C
 * bytes of page-locked host memory take a piece.
 * Stats, summed over the object's life: runs; printed rows per class, kind and haplotype; the paternal rows with a partner; bytes printed; ms of the two
 * passes (wall), of classify, emit and copy (HIP events); pass[0], pass[1]: the two passes' own stats. */
typedef struct lra_sv_combine lra_sv_combine;
struct lra_sv_combine_opts {
  uint32_t require, exclude, min_mapq, min_size, drop_contained, pos_one_based, frac_num, frac_den, filter_pass, want_text, want_values, reserved;
  uint64_t window_bytes;
  const char* aligner;
};
struct lra_sv_combine_row {
  uint64_t record, text_off, nr; int64_t start, end, svlen;
  int32_t ref_id; uint32_t qstart; uint8_t kind, strand, hap, cls; uint32_t pad;
};
struct lra_sv_combine_piece {
  uint64_t n_rows; const struct lra_sv_combine_row* rows; const char* text; uint64_t text_len; uint32_t hap, kind, cls, pad;
};
struct lra_sv_combine_stats {
  uint64_t runs, het_m_ins, het_m_del, het_p_ins, het_p_del, hom_ins, hom_del, partnered_p_ins, partnered_p_del, bytes_text;
  double ms_pass_m, ms_pass_p, ms_classify, ms_emit, ms_copy;
  struct lra_bam_svcalls_stats pass[2];
};
int lra_sv_combine_create(lra_ctx* ctx, const char* bam_m, const char* bai_m, const char* bam_p, const char* bai_p, const struct lra_sv_combine_opts* opts,
                          lra_sv_combine** out);
int lra_sv_combine_header(lra_sv_combine* d, int* n_ref, const char* const** names, const uint64_t** ref_len);
int lra_sv_combine_set_mask(lra_sv_combine* d, uint64_t n, const int32_t* ref_id, const int64_t* beg, const int64_t* end);
int lra_sv_combine_all(lra_sv_combine* d);
int lra_sv_combine_region(lra_sv_combine* d, int32_t ref_id, int64_t beg, int64_t end);
int lra_sv_combine_next(lra_sv_combine* d, struct lra_sv_combine_piece* piece);
int lra_sv_combine_stats(lra_sv_combine* d, struct lra_sv_combine_stats* out);
void lra_sv_combine_destroy(lra_sv_combine* d);
/* the reads of a snapshot whose status word is non-zero: their number; *status (optional) = the snapshot's status array [n_reads], owned by the snapshot */
uint64_t lra_map_host_flagged(const lra_map_host* snap, const uint32_t** status);
/* The record buffer of a batch as ONE device buffer -- what a rank sends to rank 0 in the single exchange step of the multi-GPU path (the
 * reference's ordered output, lra.cpp:145-166): lra_map_pack lays the same arrays out behind a 128-byte header in a context-owned buffer
 * (valid until the next pack on this context); lra_map_unpack_host turns a host copy of such a buffer (from any rank) into a snapshot for
 * lra_map_records_host.  lra_map_snapshot = pack + copy to the host + unpack.  with_blocks: the flag word above; LRA_PACK_MD appends
 * md_off u64[nA + 1] | md u8[bytes] behind the blocks (a pack whose header words 10 and 11 are 0 has none: records without MD:Z).
 * LRA_PACK_SVSIG appends, behind the MD section, sig_off u64[nA + 1] | lra_svsig_rec[sig_off[nA]] | the sequences u8[], each padded to 8 bytes,
 * header word 12 = the three parts' bytes, word 13 = 1 (both 0: no section).  lra_map_unpack_host refuses a section that is cut short or
 * inconsistent (sig_off not monotone from 0, a record's kind, block or sequence range outside its alignment / the bytes) with LRA_ERR_INVALID. */
int lra_map_pack(lra_ctx* ctx, const lra_map_result* res, int with_blocks, const void** d_buf, uint64_t* bytes);
int lra_map_unpack_host(const void* h_buf, uint64_t bytes, lra_map_host** out);
/* MapRead's second stream, svsigstrm (what Alignment::Printsvsig writes under opts.Printsvsig, Alignment.h:374-399), from a snapshot packed with
 * LRA_PACK_SVSIG: one line per signature,  chrom \t readName \t start \t end \t length \t INS|DEL \t sequence \n.  A read's lines are those of its
 * alignments in result order (job, then segment: the order of the reference's CalculateStatistics calls), an alignment's in block order;
 * (*rec_off)[n_reads + 1] gives every read's range of *text (*len bytes; both owned by the snapshot and apart from the record text, valid until
 * the snapshot is freed or the call repeated).  A read with a non-zero status word (flagged or handed back) has no lines.  n_threads as
 * lra_map_records_host; touches neither the context nor the device.  LRA_ERR_INVALID for a snapshot packed without the flag.
 * lra_map_svsig = snapshot with LRA_PACK_SVSIG, print, free; its text is owned by the context (valid until the next lra_map_svsig on it).
 * One deviation: on -CCS / -CONTIG the reference calls CalculateStatistics twice per alignment (Map_highacc.h:721, :731), so it would print every
 * signature twice, the first time from the blocks before RefineBreakpoint; here each is printed once, from the final blocks.                    */
int lra_map_svsig_host(lra_map_host* snap, const char* const* names, const char* const* chrom_names, int n_threads, const char** text, uint64_t* len,
                       const uint64_t** rec_off);
int lra_map_svsig(lra_ctx* ctx, const lra_map_result* res, const char* const* names, const char* const* chrom_names, const char** text, uint64_t* len,
                  const uint64_t** rec_off);

#ifdef __cplusplus
}
#endif
#endif /* LRA_HIP_H_ */

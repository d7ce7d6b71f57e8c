// lra_amd/csrc/map_state.h -- what the drivers of the path (mapread.hip: MapRead_lowacc, mapread_highacc.hip: MapRead_highacc) keep per context (map_reference.hip),
// and the stages both of them run the same way (map_common.hip).
#pragma once
#include <stdlib.h>
#include "common.h"
#include <string>
#include <vector>

// Host memory for a batch's record text and its largest snapshot arrays: uninitialised (a std::string / std::vector would zero 1.4 GB from one thread first) and
// handed back to a small process-wide pool instead of the allocator -- a fresh 1.4 GB mapping costs its 350 k page faults on every batch, a reused one none.
void* lra_host_pool_get(size_t bytes, size_t* cap);
void lra_host_pool_put(void* p, size_t cap);
struct lra_text_buf {
  char* p = nullptr; size_t n = 0, cap = 0;
  lra_text_buf() = default;
  lra_text_buf(const lra_text_buf&) = delete;
  lra_text_buf& operator=(const lra_text_buf&) = delete;
  ~lra_text_buf() { clear(); }
  void alloc(size_t bytes) { clear(); if (bytes) { p = (char*)lra_host_pool_get(bytes, &cap); n = p ? bytes : 0; } }
  void clear() { if (p) lra_host_pool_put(p, cap); p = nullptr; n = 0; cap = 0; }
  void swap(lra_text_buf& o) { char* tp = p; p = o.p; o.p = tp; size_t t2 = n; n = o.n; o.n = t2; t2 = cap; cap = o.cap; o.cap = t2; }
  const char* data() const { return p; }
  char* data() { return p; }
  size_t size() const { return n; }
  bool empty() const { return n == 0; }
};
template <typename T>
struct lra_pod_buf {                                                     // the same for an array of T
  lra_text_buf b;
  bool alloc(size_t count) { b.alloc(count * sizeof(T)); return count == 0 || b.data() != nullptr; }
  size_t size() const { return b.size() / sizeof(T); }
  bool empty() const { return b.empty(); }
  T* data() { return (T*)b.data(); }
  const T* data() const { return (const T*)b.data(); }
  const T& operator[](size_t i) const { return ((const T*)b.data())[i]; }
};

struct lra_map_sig {                             // what a text of lra_map_records was made from
  const void* blocks = nullptr; const void* runs = nullptr; int32_t n_reads = 0; uint64_t n_aln = 0; int32_t fmt = 0, pna = 0, hard = 0; const char* pass = nullptr;
  int32_t flagged_unaligned = 0; const void* status = nullptr;   // (the text of a flagged read depends on both)
  bool operator==(const lra_map_sig& o) const {
    return blocks == o.blocks && runs == o.runs && n_reads == o.n_reads && n_aln == o.n_aln && fmt == o.fmt && pna == o.pna && hard == o.hard && pass == o.pass &&
           flagged_unaligned == o.flagged_unaligned && status == o.status;
  }
};
struct lra_map_state {
  std::vector<uint64_t> chrom_pos;                 // Genome::header.pos, n_chrom + 1 entries
  uint64_t* d_chrom_pos = nullptr;
  void* gli_buf = nullptr; lra_local_index_result gli{};   // the genome's LocalIndex (the .gli payload), built on the device
  uint64_t* d_gso = nullptr; uint64_t n_gwin = 0;  // its seqOffsets
  int gli_window = 0, gli_k = 0, gli_w = 0;      // glIndex.localIndexWindow / k / w: what the genome's local index was built (or written by `lra index`) with
  bool borrowed = false;                           // reference data shared from another context (lra_ctx_share_reference): not freed here
  std::shared_ptr<lra_gen_cell> cell = std::make_shared<lra_gen_cell>();   // gen bumped by every loader of this context (chromosome table, local index); dead once it is destroyed
  std::shared_ptr<lra_gen_cell> owner_cell; uint64_t owner_generation = 0;  // a borrower: whose data, at which generation (see seed_state.h)
  std::vector<float> lut;                          // LogLookUpTable.h:9-15
  lra_text_buf last_text; std::vector<uint64_t> last_off; lra_map_sig last_sig;   // lra_map_records: sizing call -> filling call
  lra_text_buf sv_text; std::vector<uint64_t> sv_off;                             // lra_map_svsig: the text and read ranges of its last call
  lra_text_buf dev_text; std::vector<uint64_t> dev_off; lra_records_device_stats dev_stats{};   // lra_map_records_device: rec_off (and a fall-through's text) of its last call
  bool dev_sv = false; const char* dev_sv_ptr = nullptr; uint64_t dev_sv_len = 0;               // its SV signature text, when it was called with LRA_PACK_SVSIG: in the
  lra_text_buf dev_sv_text; std::vector<uint64_t> dev_sv_off;                                   // context's page-locked buffer, or (a fall-through's) in dev_sv_text
};

int lra_map_count_flagged(lra_ctx* ctx, lra_map_result* out);   // mapread.hip: counters.n_flagged_reads of a finished batch
int lra_map_check_shared(lra_ctx* ctx);   // map_reference.hip: borrowed reference data still current?
int lra_seed_share(lra_ctx* dst, lra_ctx* src);   // seed.hip: dst borrows src's genome and global index
int lra_seed_check_shared(lra_ctx* ctx);          // seed.hip: the same question for the genome and the global index

// The strands buffer of a batch (lra_map_result::d_strands: the reads forward, then at rc_base reverse complemented, 64 bytes of zeros) carries
// the batch's read offsets [n_reads + 1] behind it at this byte: what the record stage (LRA_PACK_MD, LRA_PACK_SVSIG) addresses the reads with once the caller's
// d_read_off may have been reused -- they travel with the strands through the two-stage handover and the passes' merges.  One copy per batch.
inline size_t lra_strands_ro_at(uint64_t rc_base) { return (size_t)((2 * rc_base + 64 + 7) & ~(uint64_t)7); }
inline size_t lra_strands_bytes(uint64_t rc_base, int n_reads) { return lra_strands_ro_at(rc_base) + ((size_t)n_reads + 1) * 8; }

// RefineBreakpoint over the consecutive SegAlignments of every job (Map_lowacc.h:586-596, Map_highacc.h:723-727); map_common.hip
int lra_refine_breakpoints(lra_ctx* ctx, uint64_t nJ, uint64_t nA, const uint64_t* d_job_aln_off, const int32_t* d_strand, const uint64_t* q_off, const int32_t* q_len,
                           const uint64_t* t_off, const int64_t* t_len, const char* strands, const char* genome, lra_refine_result* fres);
// ---- what both drivers do the same way (map_common.hip); the library's own, not part of its ABI
#pragma GCC visibility push(hidden)
inline dim3 grid(uint64_t n) { return dim3((unsigned)((n + 255) / 256)); }   // 256 threads per block over n items

// A batch may be mapped: the reference is loaded (gli_required: the genome's local index with it), a local index that is there was built with the options' k / w /
// window, and borrowed reference data is still its owner's current one.
int lra_map_ready(lra_ctx* ctx, const lra_map_opts* o, bool gli_required);
// a1-a4: the batch's seed result -- the one adopted ahead of the call (lra_seed_prefetch, lra_ctx_adopt_seed) when it was made from these reads with these parameters,
// lra_seed_batch otherwise.  defer_T > 0 (opts.defer_seed_matches): the reads with more tier-1 matches than that are handed back.
int lra_map_seed(lra_ctx* ctx, int n_reads, const char* d_seq, const uint64_t* d_read_off, int K, int W, int max_freq, uint32_t defer_T, lra_seed_result* sres);
// the strands buffer described above, in slot 57: *both
int lra_map_strands(lra_ctx* ctx, int n_reads, const char* d_seq, const uint64_t* d_read_off, uint64_t tot, char** both);
// the offsets of the 2 n_reads sequences in it, as the reads' local index wants them (slot 58), or nullptr
uint64_t* lra_map_strand_offsets(lra_ctx* ctx, int n_reads, const uint64_t* d_read_off, uint64_t tot);
// tinyOpts of LocalRefineAlignment (Map_lowacc.h:233-240, Map_highacc.h:404-409)
lra_lra_opts lra_map_lra_opts(const lra_map_opts* o);
// Every SegAlignment of a batch addressed (which read, its strand's bases, its chromosome: slots 59-63) and through IndelRefineAlignment (or, opts.skipBandedRefine,
// passed on as it is); fres.d_status kept in slot 64.  What follows -- folding that status into the reads', RefineBreakpoint, CalculateStatistics -- differs between
// the drivers and stays with them.
struct lra_map_finish {
  uint32_t* aln_read = nullptr; uint64_t* q_off = nullptr; int32_t* q_len = nullptr; uint64_t* t_off = nullptr; int64_t* t_len = nullptr;
  lra_refine_result fres{};
};
int lra_map_finish_alignments(lra_ctx* ctx, const lra_map_opts* o, int num_aln, uint64_t n_jobs, const lra_alignments_result* ares, const uint64_t* d_read_off,
                              const char* both, uint64_t tot, int endAlign, lra_map_finish* f);
// the stage results as the caller sees them
void lra_map_fill_result(lra_map_result* out, int num_aln, uint64_t n_jobs, const lra_alignments_result& ares, const lra_map_finish& f, const lra_stats_result& tres,
                         const char* both, uint64_t tot, uint8_t* job_reached, uint32_t* read_status);

double lra_wall_ms();   // a steady clock, in milliseconds
// LRA_STAGE_DBG=1: the wall time of every stage call (device work + the host-side sizing round trips around it) on stderr; does nothing otherwise
struct lra_stage_timer {
  lra_ctx* ctx; bool on; double t_prev = 0;
  explicit lra_stage_timer(lra_ctx* c);
  void operator()(const char* name);
};
#pragma GCC visibility pop

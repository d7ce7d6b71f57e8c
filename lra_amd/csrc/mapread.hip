// lra_amd/csrc/mapread.hip -- the drop-in boundary of the path: MapRead_lowacc for a batch of reads behind ONE call (gfx950 only).
//
// Replaces, for n_reads reads at a time, the body of
//     int MapRead_lowacc(LookUpTable, Read&, Genome&, genomemm, glIndex, opts, output, svsigstrm, timing, indelRefineBuffers, semaphore)
// (reference: Map_lowacc.h:33-640, entered from MapRead, MapRead.h:169-263) between "the read's bases" and "its alignments with their
// statistics" (lra_map_reads_lowacc_batch).  The stages are the library's own batched entry points, called in the reference's order; the
// only work done here is the glue the reference does with std::vector moves: keeping NumOfAnchors0 of the first sparse DP and the reads'
// status words.  This file is the low-accuracy driver only: its glue kernels, the pass (lowacc_core, lowacc_tail), the defer pass, the
// two-stage entry points with their handover, and lra_map_count_flagged.  What it shares with MapRead_highacc is in map_common.hip, the
// reference data and the presets in map_reference.hip, the per-read tail (Map_lowacc.h:600-618; lra_map_records) in map_output.hip.
#include "common.h"
#include "seed_state.h"
#include "map_state.h"
#include "map_merge.h"
#include <stdlib.h>
#include <algorithm>
#include <thread>
#include <mutex>
#include <condition_variable>
#include <functional>

namespace {

// Map_lowacc.h:86-89, :184-185: a read with a cluster of anchorfreq in (1, 2] and >= 500 matches runs its first sparse DP with anchor bonus 3
// instead of opts.initial_anchorbonus.  One wave per read over its clusters.
__global__ void __launch_bounds__(64) k_match_rate(int n_reads, const uint64_t* __restrict__ cluster_off, const uint64_t* __restrict__ c_start,
                                                   const uint64_t* __restrict__ c_end, const float* __restrict__ anchorfreq, float rate, float* __restrict__ out) {
  const int r = blockIdx.x;
  if (r >= n_reads) return;
  bool rep = false;
  for (uint64_t c = cluster_off[r] + threadIdx.x; c < cluster_off[r + 1]; c += 64) {
    const float f = anchorfreq[c];
    if (f > 1.0f && f <= 2.0f && c_end[c] - c_start[c] >= 500) rep = true;
  }
  const bool any = __ballot(rep) != 0;
  if (threadIdx.x == 0) out[r] = any ? 3.0f : rate;
}

// ---- per-read status word: the OR of every stage's per-item status (LRA_ST_* bits), so that no flagged item is emitted as an ordinary record
__global__ void k_or_status_div(uint64_t n, const uint32_t* __restrict__ status, int div, uint32_t* __restrict__ read_status) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && status[i]) atomicOr(&read_status[i / (uint64_t)div], status[i]);
}
__global__ void k_or_status_idx(uint64_t n, const uint32_t* __restrict__ status, const uint32_t* __restrict__ idx, int div, uint32_t* __restrict__ read_status) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && status[i]) atomicOr(&read_status[idx[i] / (uint32_t)div], status[i]);
}
// ---- the reads whose chains are far larger than anything else in the batch (the second, concurrent pass of lra_map_reads_lowacc_batch)
// load[r] = the number of refined matches of read r's split chains after Refine_Btwnsplitchain: what its second sparse DP will chain
__global__ void k_read_load(uint64_t n_slots, int num_aln, const uint32_t* __restrict__ n_chains, const uint64_t* __restrict__ chain_start,
                            const uint32_t* __restrict__ n_split, const uint32_t* __restrict__ sp_status, const uint64_t* __restrict__ match_off, uint32_t* __restrict__ load) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_slots) return;
  const uint64_t r = s / (uint64_t)num_aln;
  if ((uint32_t)(s % (uint64_t)num_aln) >= n_chains[r] || sp_status[s] || !n_split[s]) return;
  const uint64_t c0 = chain_start[s];
  atomicAdd(&load[r], (uint32_t)(match_off[c0 + n_split[s]] - match_off[c0]));
}
// a read above the threshold leaves this pass: its split chains are marked (every later stage skips a marked slot), and so is its status word.  The second pass gets
// the mirror image: sp2 (only the deferred reads' slots are on), their job_reached flags, a clean status array
__global__ void k_mark_deferred(int n_reads, int num_aln, const uint32_t* __restrict__ load, uint32_t threshold, uint32_t* __restrict__ sp_status,
                                uint32_t* __restrict__ read_status, uint8_t* __restrict__ deferred, uint32_t* __restrict__ sp2, uint8_t* __restrict__ reached,
                                uint8_t* __restrict__ reached2, uint32_t* __restrict__ rstat2) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_reads) return;
  const bool d = load[r] > threshold && read_status[r] == 0;
  deferred[r] = d ? 1 : 0;
  rstat2[r] = 0;
  for (int h = 0; h < num_aln; h++) {
    const uint64_t s = (uint64_t)r * num_aln + h;
    sp2[s] = d ? sp_status[s] : (uint32_t)LRA_ST_DEFERRED;
    reached2[s] = d ? reached[s] : 0;
    if (d) { sp_status[s] |= LRA_ST_DEFERRED; reached[s] = 0; }
  }
  if (d) read_status[r] |= LRA_ST_DEFERRED;
}
// opts.defer_seed_matches: the seed stage's flags become LRA_ST_DEFERRED in the reads' status words (no record is written for such a read)
__global__ void k_mark_handed_back(int n_reads, const uint8_t* __restrict__ flag, uint32_t* __restrict__ read_status, unsigned long long* count) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  const bool d = r < n_reads && flag[r];
  if (d) read_status[r] |= LRA_ST_DEFERRED;
  const unsigned long long m = __ballot(d);
  if ((threadIdx.x & (warpSize - 1)) == 0 && m) atomicAdd(count, (unsigned long long)__popcll(m));
}
__global__ void k_src_slot(uint64_t S, int na, const int32_t* __restrict__ inB, uint64_t* __restrict__ src) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const int b = inB[s / (uint64_t)na];
  src[s] = b >= 0 ? (((uint64_t)b * na + s % (uint64_t)na) | lra_merge::FROM_B) : s;
}
__global__ void k_merge_reached(uint64_t S, const uint64_t* __restrict__ src, const uint8_t* __restrict__ A, const uint8_t* __restrict__ B, uint8_t* __restrict__ out) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const uint64_t x = src[s];
  out[s] = (x & lra_merge::FROM_B) ? B[x & ~lra_merge::FROM_B] : A[x];
}
__global__ void k_merge_read_status(int R, const int32_t* __restrict__ inB, const uint32_t* __restrict__ A, const uint32_t* __restrict__ B, uint32_t* __restrict__ out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  out[r] = inB[r] >= 0 ? B[inB[r]] : A[r];
}
// per-split arrays live at chain_start[s] + k, k < n_split[s] (the split / refined-cluster numbering of chain_split.hip, refine_splitchain.hip, refine_btwn.hip)
__global__ void k_or_status_split(uint64_t n_slots, int num_aln, const uint32_t* __restrict__ n_chains, const uint64_t* __restrict__ chain_start,
                                  const uint32_t* __restrict__ n_split, const uint32_t* __restrict__ sp_status, const uint32_t* __restrict__ status,
                                  uint32_t* __restrict__ read_status) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_slots) return;
  const uint64_t r = s / (uint64_t)num_aln;
  if ((uint32_t)(s % (uint64_t)num_aln) >= n_chains[r] || sp_status[s]) return;
  uint32_t v = 0;
  for (uint64_t c = chain_start[s]; c < chain_start[s] + n_split[s]; c++) v |= status[c];
  if (v) atomicOr(&read_status[r], v);
}
// Which primary chains p reach `alignments.resize(alignments.size() + 1)` (Map_lowacc.h:574): the chain exists, SPLITChain +
// RemoveSpuriousSplitChain left a split chain (:263-267) and the refined clusters hold at least one match (:486-491).  A chain that
// does not ends the loop over p (p > 0: break) or the read (p == 0: unaligned); one that does adds a SegAlignmentGroup even when
// LocalRefineAlignment then produces no SegAlignment.
__global__ void k_job_reached(uint64_t n_slots, int num_aln, const uint32_t* __restrict__ n_chains, const uint64_t* __restrict__ chain_start,
                              const uint32_t* __restrict__ n_split, const uint32_t* __restrict__ sp_status, const uint64_t* __restrict__ match_off,
                              uint8_t* __restrict__ reached) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_slots) return;
  bool ok = (uint32_t)(s % (uint64_t)num_aln) < n_chains[s / (uint64_t)num_aln] && !sp_status[s] && n_split[s] > 0;
  if (ok) { const uint64_t cs = chain_start[s]; ok = match_off[cs + n_split[s]] > match_off[cs]; }
  reached[s] = ok ? 1 : 0;
}

// The loop over p ENDS at the first chain that does not reach :574 (p > 0: break, :267 / :491; p == 0: the read is unaligned): the chains behind it are never mapped.
// Their slots are switched off here (every later stage skips a marked slot, as for a deferred read), so the device's result holds no alignment the reference would not
// have made -- lra_map_records* ends a read's loop at the same place either way.
__global__ void k_cut_behind_unreached(int n_reads, int num_aln, uint32_t* __restrict__ sp_status, uint8_t* __restrict__ reached) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_reads) return;
  bool off = false;
  for (int h = 0; h < num_aln; h++) {
    const uint64_t s = (uint64_t)r * num_aln + h;
    if (off) { if (reached[s]) { reached[s] = 0; sp_status[s] |= (uint32_t)LRA_ST_DEFERRED; } }
    else if (!reached[s]) off = true;
  }
}

// which (strand, read) sequences of the forward + reverse-complement buffer Refine_splitchain will look up: those a split chain lies on
__global__ void k_mark_strands(uint64_t n_slots, int num_aln, int n_reads, const uint32_t* __restrict__ n_split, const uint64_t* __restrict__ chain_start,
                               const uint8_t* __restrict__ sp_strand, const uint32_t* __restrict__ status, uint8_t* __restrict__ active) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_slots || status[s]) return;
  const uint32_t r = (uint32_t)(s / (uint64_t)num_aln);
  for (uint32_t k = 0; k < n_split[s]; k++) active[(sp_strand[chain_start[s] + k] ? n_reads : 0) + r] = 1;
}

// tuple words the local compare stage reads (the algorithmic bytes of local_compare): sum over tasks of both list lengths
__global__ void k_task_words(uint64_t n, const uint64_t* __restrict__ qlo, const uint64_t* __restrict__ qhi, const uint64_t* __restrict__ tlo,
                             const uint64_t* __restrict__ thi, unsigned long long* sum) {
  unsigned long long v = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) v += (qhi[i] - qlo[i]) + (thi[i] - tlo[i]);
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(sum, v);
}

}  // namespace

extern "C" int lra_match_rate_batch(lra_ctx* ctx, const lra_cluster_result* clusters, float initial_anchorbonus, const float** d_rate) {
  if (!ctx || !clusters || !d_rate) return LRA_ERR_INVALID;
  *d_rate = nullptr;
  const int n_reads = clusters->n_reads;
  float* rate = (float*)lra_ensure(ctx, 80, ((size_t)n_reads + 1) * 4);
  if (!rate) return LRA_ERR_NOMEM;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (n_reads) hipLaunchKernelGGL(k_match_rate, dim3(n_reads), dim3(64), 0, ctx->stream, n_reads, clusters->d_cluster_off, clusters->d_c_start, clusters->d_c_end,
                                  clusters->d_c_anchorfreq, initial_anchorbonus, rate);
  *d_rate = rate;
  return LRA_OK;
}

// One pass of MapRead_lowacc over a batch.  defer_threshold > 0: the reads with more refined matches than that after Refine_Btwnsplitchain leave the pass there (no
// alignments, LRA_ST_DEFERRED in their status word); *deferred lists them and on_deferred runs as soon as the list is known.
// What the stages behind the split point need from the ones in front of it (device pointers into the first pass's buffers, which it leaves alone from there on)
struct LowaccTailIn {
  int n_reads = 0, num_aln = 1; uint64_t n_slots = 0, tot = 0;
  const uint64_t* d_read_off = nullptr; const char* d_seq = nullptr; const char* both = nullptr;
  const uint32_t* slot_n0 = nullptr;
  lra_merge_result mres;
  uint8_t* job_reached = nullptr; uint32_t* read_status = nullptr;
  lra_map_counters counters;
};
static int lowacc_tail(lra_ctx* ctx, const LowaccTailIn& in, const lra_map_opts* o, lra_map_result* out);

// A batch between its two halves (lra_map_reads_lowacc_front / _back): what the tail needs, and a queue of ONE batch between the threads of the two halves.
// The front half writes the batch it hands over (MergeChain .. TrimOverlappedAnchors' results, the reads with their reverse complements, the chains' NumOfAnchors0, the
// slots reached, the status words) into one of two sets of buffers -- the handover contexts hand[0 / 1], taken in turn -- so it never waits for the back half that is
// RUNNING, only for the batch before its own to have been taken: when batch i - 1 has been taken, batch i - 2 has been released, and set i % 2 is free.
struct lra_handover {
  std::mutex mu; std::condition_variable cv;
  bool pending = false;    // a batch is handed over, its back half not yet started
  bool busy = false;       // the back half runs, or its result is still in use (until lra_map_back_release)
  uint64_t seq = 0;        // batches handed over so far (error batches do not count: they use no buffers)
  lra_ctx* hand[2] = {nullptr, nullptr};   // owned through the companion's child chain (destroyed and timed with it)
  LowaccTailIn in;
  int rc = LRA_OK;         // pending only: the front half of this batch FAILED with this code (nothing to run: the back call returns it)
  std::string err;
};
void lra_handover_free(lra_ctx* ctx) { delete ctx->handover; ctx->handover = nullptr; }
bool lra_handover_idle(lra_ctx* ctx) {                                     // lra_ctx_release_buffers: nothing handed over and not taken, no back half running or unreleased
  lra_handover* H = ctx->handover;
  if (!H) return true;
  std::lock_guard<std::mutex> lk(H->mu);
  return !H->pending && !H->busy;
}
static lra_handover* handover_of(lra_ctx* ctx) {                         // (the two halves' threads may both be the first to ask)
  static std::mutex make;
  std::lock_guard<std::mutex> lk(make);
  if (!ctx->handover) ctx->handover = new lra_handover();
  return ctx->handover;
}

static int child_refresh(lra_ctx* ctx);
static int lowacc_core(lra_ctx* ctx, int n_reads, const char* d_seq, const uint64_t* d_read_off, uint64_t total_bases, const lra_map_opts* o, lra_map_result* out,
                       uint32_t defer_threshold, std::vector<uint32_t>* deferred, lra_ctx* second, LowaccTailIn* second_in, const std::function<int()>& on_deferred,
                       lra_handover* H = nullptr) {
  memset(out, 0, sizeof *out);
  lra_map_state* m = ctx->map;
  out->n_reads = n_reads;
  if (n_reads == 0) return LRA_OK;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  uint32_t* read_status = (uint32_t*)lra_ensure(ctx, 81, ((size_t)n_reads + 1) * 4);
  if (!read_status) return LRA_ERR_NOMEM;
  LRA_HIP_CHECK(ctx, hipMemsetAsync(read_status, 0, (size_t)n_reads * 4, st));
  const uint64_t* CH = m->chrom_pos.data();
  const int nCh = (int)m->chrom_pos.size() - 1;
  const char* genome = (const char*)ctx->seed->genome;
  const uint64_t tot = total_bases;
  int rc;
  lra_stage_timer stage(ctx);
  // a1-a4
  lra_seed_result sres;
  // opts.defer_seed_matches: the reads with more tier-1 matches than that are handed back (the seed stage empties their match lists: no later stage sees them)
  const uint32_t seedT = o->defer_seed_matches > 0 ? (uint32_t)o->defer_seed_matches : 0;
  if ((rc = lra_map_seed(ctx, n_reads, d_seq, d_read_off, o->globalK, o->globalW, o->globalMaxFreq, seedT, &sres))) return rc;   // (nothing on this path reads opts.globalW after it)
  uint64_t n_handed_back = 0;
  if (seedT) {
    unsigned long long* dcnt = (unsigned long long*)lra_ensure(ctx, 191, 64);
    if (!dcnt) return LRA_ERR_NOMEM;
    LRA_HIP_CHECK(ctx, hipMemsetAsync(dcnt, 0, 8, st));
    hipLaunchKernelGGL(k_mark_handed_back, grid((uint64_t)n_reads), dim3(256), 0, st, n_reads, (const uint8_t*)ctx->seed->defer_flag, read_status, dcnt);
    unsigned long long h = 0;
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&h, dcnt, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    n_handed_back = h;
  }
  stage("seed");
  // a5, a7
  lra_cluster_result cres;
  if ((rc = lra_clean_matches_batch(ctx, &o->clean, CH, nCh, &cres))) return rc;
  stage("clean");
  lra_extend_result eres;
  if ((rc = lra_linear_extend_batch(ctx, o->globalK, d_seq, d_read_off, &eres))) return rc;
  stage("linear_extend");
  // a8: the primary chains (Map_lowacc.h:184-188); match_rate = 3 for reads with a repetitive cluster (:86-89)
  const float* match_rate = nullptr;
  if ((rc = lra_match_rate_batch(ctx, &cres, o->sdp.rate, &match_rate))) return rc;
  lra_chain_result chres;
  if ((rc = lra_sparse_dp_batch(ctx, n_reads, cres.d_cluster_off, eres.d_e_start, eres.d_e_count, cres.d_c_strand, eres.d_e_qpos, eres.d_e_tpos, eres.d_e_len,
                                d_read_off, match_rate, &o->sdp, &chres))) return rc;
  stage("sdp#A");
  const int num_aln = chres.num_aln;
  const uint64_t n_slots = (uint64_t)n_reads * (uint64_t)num_aln;
  hipLaunchKernelGGL(k_or_status_div, grid(n_reads), dim3(256), 0, st, (uint64_t)n_reads, chres.d_status, 1, read_status);
  // chains[p].NumOfAnchors0 (the second sparse DP reuses the first one's buffers)
  uint32_t* slot_n0 = (uint32_t*)lra_ensure(ctx, 56, (n_slots + 1) * 4);
  if (!slot_n0) return LRA_ERR_NOMEM;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(slot_n0, chres.d_chain_len, n_slots * 4, hipMemcpyDeviceToDevice, st));
  // a9
  lra_split_result spres;
  if ((rc = lra_split_chains_batch(ctx, &chres, CH, nCh, o->splitdist, o->bypassClustering, &spres))) return rc;
  stage("split_chains");
  hipLaunchKernelGGL(k_or_status_div, grid(n_slots), dim3(256), 0, st, n_slots, spres.d_status, num_aln, read_status);
  // a10: the reads forward, then reverse complemented, in one buffer + its local index (Map_lowacc.h:246-250)
  char* both = nullptr;
  if ((rc = lra_map_strands(ctx, n_reads, d_seq, d_read_off, tot, &both))) return rc;
  const uint64_t* off2 = lra_map_strand_offsets(ctx, n_reads, d_read_off, tot);
  if (!off2) return LRA_ERR_NOMEM;
  // the reference indexes both strands of every read; only the strands with a split chain are ever looked up, so only those get tuples
  uint8_t* active = (uint8_t*)lra_ensure(ctx, 65, 2 * (size_t)n_reads + 64);
  if (!active) return LRA_ERR_NOMEM;
  LRA_HIP_CHECK(ctx, hipMemsetAsync(active, 0, 2 * (size_t)n_reads, st));
  hipLaunchKernelGGL(k_mark_strands, grid(n_slots), dim3(256), 0, st, n_slots, num_aln, n_reads, spres.d_n_split, chres.d_chain_start,
                     spres.d_sp_strand, spres.d_status, active);
  lra_local_index_result rli;
  if ((rc = lra_local_index_masked_batch(ctx, 2 * n_reads, both, off2, active, o->localK, o->localW, o->localIndexWindow, o->localMaxFreq, &rli))) return rc;
  stage("read local index");
  lra_rsc_opts ro; ro.window = o->window; ro.smallK = o->localK; ro.K = o->globalK; ro.limitrefine = 1; ro.max_freq = o->localMaxFreq; ro.local_window = o->localIndexWindow;
  lra_refined_result rres;
  if ((rc = lra_refine_splitchain_batch(ctx, &chres, &spres, d_read_off, CH, nCh, &rli, m->n_gwin, m->d_gso, m->gli.d_tuple_bnd, m->gli.d_tuples, &ro, &rres))) return rc;
  stage("refine_splitchain");
  uint64_t task_words = 0;
  if (rres.n_tasks) {
    unsigned long long* d_sum = (unsigned long long*)lra_scratch(ctx, 3, 256);
    if (!d_sum) return LRA_ERR_NOMEM;
    LRA_HIP_CHECK(ctx, hipMemsetAsync(d_sum, 0, 8, st));
    hipLaunchKernelGGL(k_task_words, dim3((unsigned)std::min<uint64_t>((rres.n_tasks + 255) / 256, 1024)), dim3(256), 0, st, rres.n_tasks, rres.d_task_q_lo,
                       rres.d_task_q_hi, rres.d_task_t_lo, rres.d_task_t_hi, d_sum);
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&task_words, d_sum, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  }
  // a11 callers
  lra_btwn_opts bo; bo.K = o->localK; bo.W = o->localW; bo.refineSpaceDist = o->refineSpaceDist; bo.anchorstoosparse = o->anchorstoosparse;
  bo.match = o->localMatch; bo.mismatch = o->localMismatch; bo.indel = o->localIndel; bo.max_freq = o->localMaxFreq;
  lra_btwn_result bres;
  if ((rc = lra_refine_btwn_splitchain_batch(ctx, &chres, &spres, &rres, d_read_off, both, tot, genome, CH, nCh, &bo, &bres))) return rc;
  stage("refine_btwn_splitchain");
  uint8_t* job_reached = (uint8_t*)lra_ensure(ctx, 82, n_slots + 64);
  if (!job_reached) return LRA_ERR_NOMEM;
  hipLaunchKernelGGL(k_job_reached, grid(n_slots), dim3(256), 0, st, n_slots, num_aln, chres.d_n_chains, chres.d_chain_start, spres.d_n_split, spres.d_status,
                     bres.d_match_off, job_reached);
  if (rres.n_frags) hipLaunchKernelGGL(k_or_status_split, grid(n_slots), dim3(256), 0, st, n_slots, num_aln, chres.d_n_chains, chres.d_chain_start, spres.d_n_split,
                                       spres.d_status, rres.d_status, read_status);
  hipLaunchKernelGGL(k_cut_behind_unreached, grid((uint64_t)n_reads), dim3(256), 0, st, n_reads, num_aln, (uint32_t*)spres.d_status, job_reached);
  // counters of the stages so far
  lra_map_counters cnt0; memset(&cnt0, 0, sizeof cnt0);
  cnt0.n_minimizers = sres.n_minimizers; cnt0.n_matches = sres.n_matches; cnt0.n_clusters = cres.n_clusters; cnt0.n_sdp_anchors = chres.n_frags; cnt0.n_sdp_points = chres.n_points;
  cnt0.n_sdp_entries = chres.n_subproblem_entries; cnt0.n_local_tuples = rli.n_tuples; cnt0.n_local_tasks = rres.n_tasks; cnt0.n_local_task_words = task_words; cnt0.n_local_pairs = rres.n_pairs;
  cnt0.n_handed_back_reads = n_handed_back; cnt0.n_refined_matches = rres.n_matches; cnt0.n_btwn_problems = bres.n_problems; cnt0.n_btwn_rounds = bres.n_rounds; cnt0.n_refined_after_btwn = bres.n_matches;
  LowaccTailIn in;
  in.n_reads = n_reads; in.num_aln = num_aln; in.n_slots = n_slots; in.tot = tot; in.d_read_off = d_read_off; in.d_seq = d_seq; in.both = both; in.slot_n0 = slot_n0;
  in.job_reached = job_reached; in.read_status = read_status; in.counters = cnt0;
  if (const char* dumpPath = getenv("LRA_LOAD_DUMP")) {                  // analysis: per read, the tier-1 matches and the refined matches its second sparse DP will chain
    uint32_t* load = (uint32_t*)lra_ensure(ctx, 181, ((size_t)n_reads + 1) * 4);
    if (!load) return LRA_ERR_NOMEM;
    LRA_HIP_CHECK(ctx, hipMemsetAsync(load, 0, (size_t)n_reads * 4, st));
    hipLaunchKernelGGL(k_read_load, grid(n_slots), dim3(256), 0, st, n_slots, num_aln, chres.d_n_chains, chres.d_chain_start, spres.d_n_split, spres.d_status, bres.d_match_off, load);
    std::vector<uint32_t> hl((size_t)n_reads), hs((size_t)n_slots); std::vector<uint64_t> hm((size_t)n_reads + 1), hq((size_t)n_reads + 1);
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(hl.data(), load, (size_t)n_reads * 4, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(hs.data(), spres.d_n_split, (size_t)n_slots * 4, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(hm.data(), sres.d_match_off, ((size_t)n_reads + 1) * 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(hq.data(), sres.d_mm_off, ((size_t)n_reads + 1) * 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (FILE* f = fopen(dumpPath, "wb")) {
      const uint32_t hdr[2] = {(uint32_t)n_reads, (uint32_t)num_aln};
      fwrite(hdr, 4, 2, f); fwrite(hm.data(), 8, hm.size(), f); fwrite(hq.data(), 8, hq.size(), f); fwrite(hl.data(), 4, hl.size(), f); fwrite(hs.data(), 4, hs.size(), f);
      fclose(f);
    }
  }
  // ---- the split point: reads with more refined matches than the threshold go on in the second context (from here: MergeChain onwards), beside this pass
  if (defer_threshold && deferred && second && second_in) {
    uint32_t* load = (uint32_t*)lra_ensure(ctx, 181, ((size_t)n_reads + 1) * 4);
    uint8_t* dflag = (uint8_t*)lra_ensure(ctx, 182, (size_t)n_reads + 64);
    if (!load || !dflag) return LRA_ERR_NOMEM;
    LRA_HIP_CHECK(ctx, hipMemsetAsync(load, 0, (size_t)n_reads * 4, st));
    hipLaunchKernelGGL(k_read_load, grid(n_slots), dim3(256), 0, st, n_slots, num_aln, chres.d_n_chains, chres.d_chain_start, spres.d_n_split, spres.d_status, bres.d_match_off, load);
    uint32_t* sp2 = (uint32_t*)lra_ensure(second, 183, (n_slots + 1) * 4);    // the second pass's view of the split chains: everything but the deferred reads' slots is off
    uint8_t* reached2 = (uint8_t*)lra_ensure(second, 82, n_slots + 64);
    uint32_t* rstat2 = (uint32_t*)lra_ensure(second, 81, ((size_t)n_reads + 1) * 4);
    if (!sp2 || !reached2 || !rstat2) return LRA_ERR_NOMEM;
    hipLaunchKernelGGL(k_mark_deferred, grid(n_reads), dim3(256), 0, st, n_reads, num_aln, (const uint32_t*)load, defer_threshold, (uint32_t*)spres.d_status, read_status, dflag,
                       sp2, job_reached, reached2, rstat2);
    std::vector<uint8_t> hf((size_t)n_reads);
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(hf.data(), dflag, (size_t)n_reads, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    deferred->clear();
    for (int r = 0; r < n_reads; r++) if (hf[r]) deferred->push_back((uint32_t)r);
    if (!deferred->empty()) {
      // MergeChain .. TrimOverlappedAnchors of the deferred reads' chains, into the second context's buffers but queued on THIS stream: it reads the first sparse DP's
      // arrays, which this pass's second sparse DP is about to reuse
      lra_split_result spB = spres; spB.d_status = sp2;
      const hipStream_t keep = second->stream;
      second->stream = st;
      rc = lra_merge_extend_batch(second, &chres, &spB, &bres, d_seq, d_read_off, genome, CH, nCh, o->localK, &second_in->mres);
      second->stream = keep;
      if (rc) return lra_set_err(ctx, rc, "second pass, MergeChain: %s", second->err.c_str());
      LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
      { const lra_merge_result keepM = second_in->mres; *second_in = in; second_in->mres = keepM; second_in->job_reached = reached2; second_in->read_status = rstat2; }
      if (on_deferred && (rc = on_deferred())) return rc;
    }
    stage("deferred reads");
  }
  if (H) {
    // The front half ends here (lra_map_reads_lowacc_front): MergeChain .. TrimOverlappedAnchors write into the handover buffers of this batch's turn (queued on this
    // stream: they read the first sparse DP's and the refinement's arrays), and the four buffers of this half that the tail reads -- the reads with their reverse
    // complements, the chains' NumOfAnchors0, the slots reached, the reads' status words -- change owner with that set's (no copy).  Not before the batch before this one
    // has been TAKEN by a back call (then the set's last user, the batch before that, has been released); the back half that is running is not waited for.
    const double tw0 = lra_wall_ms();
    { std::unique_lock<std::mutex> lk(H->mu); H->cv.wait(lk, [&] { return !H->pending; }); }
    if (getenv("LRA_TWO_STAGE_DBG")) fprintf(stderr, "[two-stage] front half waited %.0f ms for the batch before it to be taken\n", lra_wall_ms() - tw0);
    lra_ctx* hs = H->hand[H->seq & 1];
    for (int slot : {56, 57, 81, 82}) { std::swap(ctx->gbuf[slot], hs->gbuf[slot]); std::swap(ctx->gbytes[slot], hs->gbytes[slot]); }
    hs->stream = st;                                                       // (a handover context has no stream of its own: its one stage runs on the front half's)
    // (the stage's work arrays -- per refined match, dead when it returns -- and its sort's scratch are this context's, lent for the call: one set, not one per handover context)
    auto lend = [&]() { std::swap(ctx->gbuf[100], hs->gbuf[100]); std::swap(ctx->gbytes[100], hs->gbytes[100]); std::swap(ctx->scratch[2], hs->scratch[2]); std::swap(ctx->scratch_bytes[2], hs->scratch_bytes[2]); };
    lend();
    rc = lra_merge_extend_batch(hs, &chres, &spres, &bres, d_seq, d_read_off, genome, CH, nCh, o->localK, &in.mres);
    lend();
    if (rc) return lra_set_err(ctx, rc, "MergeChain into the handover buffers: %s", hs->err.c_str());
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    stage("merge_extend");
    { std::lock_guard<std::mutex> lk(H->mu); H->in = in; H->rc = LRA_OK; H->pending = true; H->seq++; }
    H->cv.notify_all();
    return LRA_OK;
  }
  // a9 MergeChain, a7 second pass (Map_lowacc.h:411-476)
  if ((rc = lra_merge_extend_batch(ctx, &chres, &spres, &bres, d_seq, d_read_off, genome, CH, nCh, o->localK, &in.mres))) return rc;
  stage("merge_extend");
  return lowacc_tail(ctx, in, o, out);
}

// a8 second sparse DP, a13, a14, a16 (Map_lowacc.h:477-599) on the merged clusters of `in`
static int lowacc_tail(lra_ctx* ctx, const LowaccTailIn& in, const lra_map_opts* o, lra_map_result* out) {
  lra_map_state* m = ctx->map;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int n_reads = in.n_reads, num_aln = in.num_aln; const uint64_t tot = in.tot;
  const uint64_t* d_read_off = in.d_read_off; const char* both = in.both; const uint32_t* slot_n0 = in.slot_n0;
  const lra_merge_result& mres = in.mres;
  uint8_t* job_reached = in.job_reached; uint32_t* read_status = in.read_status;
  const uint64_t* CH = m->chrom_pos.data();
  const int nCh = (int)m->chrom_pos.size() - 1;
  const char* genome = (const char*)ctx->seed->genome;
  int rc;
  lra_stage_timer stage(ctx);
  out->n_reads = n_reads;
  lra_sdp_opts s2 = o->sdp; s2.mode = 1; s2.rate = o->second_anchorbonus;      // SparseDP :2287 with opts.second_anchorbonus (Options.h:221)
  lra_chain_result ch2;
  if ((rc = lra_sparse_dp_batch(ctx, (int)mres.n_groups, mres.d_iota, mres.d_anchor_off, mres.d_count, mres.d_strand, mres.d_q, mres.d_t, mres.d_len, mres.d_iota,
                                nullptr, &s2, &ch2))) return rc;
  stage("sdp#2");
  if (mres.n_groups) hipLaunchKernelGGL(k_or_status_idx, grid(mres.n_groups), dim3(256), 0, st, mres.n_groups, ch2.d_status, mres.d_group_slot, num_aln, read_status);
  // a13
  lra_local_refine_inputs inp;
  if ((rc = lra_local_refine_inputs_batch(ctx, num_aln, slot_n0, &mres, &ch2, &inp))) return rc;
  stage("local_refine_inputs");
  const lra_lra_opts lo = lra_map_lra_opts(o);
  lra_alignments_result ares;
  if ((rc = lra_local_refine_batch(ctx, inp.n_jobs, inp.d_job_chain_off, inp.d_job_read, inp.d_job_h, inp.n_chains, inp.d_chain_anchor_off, inp.d_chain_strand,
                                   inp.d_chain_chrom, inp.d_chain_value, inp.d_chain_n0, inp.d_chain_n1, inp.n_anchors, inp.d_q, inp.d_t, inp.d_len, d_read_off,
                                   both, tot, genome, CH, nCh, &lo, &ares))) return rc;
  stage("local_refine");
  const uint64_t nA = ares.n_alignments, nJ = ares.n_jobs;
  if (nJ) hipLaunchKernelGGL(k_or_status_div, grid(nJ), dim3(256), 0, st, nJ, ares.d_status, num_aln, read_status);
  // a14, a16 on every SegAlignment (Map_lowacc.h:582-599)
  lra_map_finish f;
  if ((rc = lra_map_finish_alignments(ctx, o, num_aln, nJ, &ares, d_read_off, both, tot, 0, &f))) return rc;
  lra_refine_result& fres = f.fres;
  lra_stats_result tres; memset(&tres, 0, sizeof tres);
  if (nA) {
    if (fres.d_status) hipLaunchKernelGGL(k_or_status_idx, grid(nA), dim3(256), 0, st, nA, (const uint32_t*)fres.d_status, f.aln_read, 1, read_status);
    if (o->refineBreakpoint && (rc = lra_refine_breakpoints(ctx, nJ, nA, ares.d_job_aln_off, ares.d_strand, f.q_off, f.q_len, f.t_off, f.t_len, both, genome, &fres))) return rc;
    stage("indel_refine (+breakpoints)");
    if ((rc = lra_calculate_statistics_batch(ctx, (int)nA, fres.d_blocks, fres.d_block_off, both, f.q_off, f.q_len, genome, f.t_off, m->lut.data(), (int)m->lut.size(), &tres)))
      return rc;
    stage("statistics");
  }
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  LRA_HIP_CHECK(ctx, hipGetLastError());
  lra_map_fill_result(out, num_aln, nJ, ares, f, tres, both, tot, job_reached, read_status);
  if (getenv("LRA_MEM_DBG")) {
    size_t tot = 0;
    for (int i = 0; i < 192; i++) { tot += ctx->gbytes[i]; if (ctx->gbytes[i] > (size_t(1) << 30)) fprintf(stderr, "[mem] gbuf %d %.1f GB\n", i, ctx->gbytes[i] / 1e9); }
    for (int i = 0; i < 4; i++) { tot += ctx->scratch_bytes[i]; fprintf(stderr, "[mem] scratch %d %.1f GB\n", i, ctx->scratch_bytes[i] / 1e9); }
    fprintf(stderr, "[mem] aux %.1f out %.1f GB total %.1f GB\n", ctx->aux_bytes / 1e9, ctx->out_bytes / 1e9, (tot + ctx->aux_bytes + ctx->out_bytes) / 1e9);
  }
  // counters of the batch (what bench.py prices the roofline with)
  lra_map_counters& c = out->counters;
  c = in.counters;
  c.n_merged_clusters = mres.n_groups; c.n_sdp2_anchors = mres.n_anchors; c.n_sdp2_entries = ch2.n_subproblem_entries; c.n_a13_blocks = ares.n_blocks;
  c.n_large_spaces = ares.n_big; c.n_segments = fres.n_segments; c.n_rows = fres.n_rows; c.n_cells = fres.n_cells; c.n_aog = fres.n_aog;
  return LRA_OK;
}

// lra_map_reads_lowacc_batch: the pass above.  With opts.defer_matches > 0 the batch's most repetitive reads -- a read inside a satellite array ends up with tens of
// thousands of refined matches where a typical 30 kb read has three thousand, and its second sparse DP keeps one workgroup busy for half a second -- leave the pass after
// Refine_Btwnsplitchain and go on, from MergeChain, in a child context on its own lowest-priority stream and host thread BESIDE the rest of the pass; the two results
// are merged on the device (a read's alignments do not depend on which pass computed them: tests/test_mapread.py ont-defer*).  Off in the presets: on this device it is
// no gain at any threshold -- the repetitive reads' work is throughput that the pass's own launches already overlap, not an idle tail.
namespace {
__global__ void k_count_flagged(int n, const uint32_t* __restrict__ st, unsigned long long* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long m = __ballot(i < n && st[i] != 0 && st[i] != (uint32_t)LRA_ST_DEFERRED);   // (a handed-back read is not a flagged one: counters.n_handed_back_reads)
  if ((threadIdx.x & (warpSize - 1)) == 0 && m) atomicAdd(out, (unsigned long long)__popcll(m));
}
}  // namespace
// counters.n_flagged_reads of a finished batch: the reads whose status word is non-zero get no alignment record (lra_map_records*), the caller must know how many
int lra_map_count_flagged(lra_ctx* ctx, lra_map_result* out) {
  out->counters.n_flagged_reads = 0;
  if (!out->d_read_status || out->n_reads <= 0) return LRA_OK;
  unsigned long long* d = (unsigned long long*)lra_ensure(ctx, 191, 64);
  if (!d) return LRA_ERR_NOMEM;
  LRA_HIP_CHECK(ctx, hipMemsetAsync(d, 0, 8, ctx->stream));
  hipLaunchKernelGGL(k_count_flagged, dim3((out->n_reads + 255) / 256), dim3(256), 0, ctx->stream, out->n_reads, out->d_read_status, d);
  unsigned long long h = 0;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&h, d, 8, hipMemcpyDeviceToHost, ctx->stream));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  out->counters.n_flagged_reads = h;
  return LRA_OK;
}

// The context's companion (a batch's second, concurrent pass; the back half of two-stage batches): a context of its own -- stream, work buffers -- that borrows this
// one's reference data.  `lowest`: its streams at the device's lowest priority (the second pass fills the gaps the first one leaves; at equal priority the two passes'
// queues slow each other down far beyond the work involved, measured); otherwise at LRA_BACK_PRIORITY (default: the device's highest -- the back half of a batch is the longer one, the front half of the next fills in).
static int child_create(lra_ctx* ctx, bool lowest) {
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (!ctx->child) {
    lra_ctx* c = nullptr;
    int rc = lra_ctx_create(ctx->device, &c);
    if (rc) return lra_set_err(ctx, rc, "companion context");
    if ((rc = lra_ctx_share_reference(c, ctx))) { lra_ctx_destroy(c); return lra_set_err(ctx, rc, "companion context: sharing the reference"); }
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    int prio = least;
    if (!lowest) { prio = getenv("LRA_BACK_PRIORITY") ? atoi(getenv("LRA_BACK_PRIORITY")) : greatest; prio = std::max(greatest, std::min(least, prio)); }
    c->low_priority = true; c->prio = prio;                               // (low_priority: the context keeps the priority it was made with, lra_ctx_set_stream)
    if (hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio) != hipSuccess) { c->stream = nullptr; lra_ctx_destroy(c); return lra_set_err(ctx, LRA_ERR_HIP, "companion stream"); }
    c->owns_stream = true; c->timing = ctx->timing;
    ctx->child = c;
  }
  return LRA_OK;
}
// The companion's view of the parent's reference data (the parent's reference may have been loaded / built again since the last batch).  Writes the companion's
// state: only while nothing runs on the companion (two-stage batches: the front half calls it once it holds the back context, never while a back half may be running).
static int child_refresh(lra_ctx* ctx) {
  lra_ctx* c = ctx->child;
  int rc = lra_seed_share(c, ctx);
  if (rc) return lra_set_err(c, rc, "companion context: sharing the reference");   // (on the companion: in two-stage batches this runs on the back halves' thread)
  lra_map_state* d = c->map; const lra_map_state* s = ctx->map;
  d->chrom_pos = s->chrom_pos; d->d_chrom_pos = s->d_chrom_pos; d->gli_buf = s->gli_buf; d->gli = s->gli; d->d_gso = s->d_gso; d->n_gwin = s->n_gwin;
  d->gli_window = s->gli_window; d->gli_k = s->gli_k; d->gli_w = s->gli_w; d->lut = s->lut; d->borrowed = true;
  d->owner_cell = s->borrowed ? s->owner_cell : s->cell; d->owner_generation = s->borrowed ? s->owner_generation : s->cell->gen.load();
  return LRA_OK;
}
static int ensure_child(lra_ctx* ctx, bool lowest) {
  int rc = child_create(ctx, lowest);
  if (rc) return rc;
  if ((rc = child_refresh(ctx))) return lra_set_err(ctx, rc, "%s", ctx->child->err.c_str());
  return LRA_OK;
}

static int lowacc_batch_impl(lra_ctx* ctx, int n_reads, const char* d_seq, const uint64_t* d_read_off, uint64_t total_bases, const lra_map_opts* o, lra_map_result* out);
extern "C" int lra_map_reads_lowacc_batch(lra_ctx* ctx, int n_reads, const char* d_seq, const uint64_t* d_read_off, uint64_t total_bases,
                                          const lra_map_opts* o, lra_map_result* out) {
  int rc = lowacc_batch_impl(ctx, n_reads, d_seq, d_read_off, total_bases, o, out);
  if (rc == LRA_OK && out && n_reads > 0) rc = lra_map_count_flagged(ctx, out);
  return rc;
}
static int lowacc_batch_impl(lra_ctx* ctx, int n_reads, const char* d_seq, const uint64_t* d_read_off, uint64_t total_bases, const lra_map_opts* o, lra_map_result* out) {
  if (!ctx || !o || !out || n_reads < 0) return LRA_ERR_INVALID;
  memset(out, 0, sizeof *out);
  { int rcs = lra_map_ready(ctx, o, true); if (rcs) return rcs; }
  lra_map_state* m = ctx->map;
  out->n_reads = n_reads;
  m->last_text.clear(); m->last_sig = lra_map_sig{};         // a sizing call of lra_map_records for an earlier batch is void now
  ctx->pipelined = false;                                    // (the one call: nothing runs beside it)
  if (n_reads == 0) return LRA_OK;
  const uint32_t threshold = o->defer_matches > 0 ? (uint32_t)o->defer_matches : 0;
  const std::function<int()> none;
  if (!threshold) return lowacc_core(ctx, n_reads, d_seq, d_read_off, total_bases, o, out, 0, nullptr, nullptr, nullptr, none);
  { int rcc = ensure_child(ctx, true); if (rcc) return rcc; }
  std::vector<uint32_t> picked;
  std::thread second;
  int rc2 = LRA_OK;
  LowaccTailIn in2;
  lra_map_result o2; memset(&o2, 0, sizeof o2);
  const bool ddbg = getenv("LRA_DEFER_DBG") != nullptr;
  const double t0 = lra_wall_ms();
  double t_split = 0, t_second = 0;
  auto start_second = [&]() -> int {
    t_split = lra_wall_ms();
    second = std::thread([&, c = ctx->child]() {
      rc2 = lowacc_tail(c, in2, o, &o2);
      t_second = lra_wall_ms();
    });
    return LRA_OK;
  };
  int rc = lowacc_core(ctx, n_reads, d_seq, d_read_off, total_bases, o, out, threshold, &picked, ctx->child, &in2, start_second);
  const double t1 = lra_wall_ms();
  if (second.joinable()) second.join();
  if (ddbg) fprintf(stderr, "[defer] %d reads; split at %.0f ms, second pass done at %.0f ms, first pass done at %.0f ms\n", (int)picked.size(), t_split - t0, t_second - t0, t1 - t0);
  if (rc) return rc;
  if (picked.empty()) return LRA_OK;
  if (rc2) return lra_set_err(ctx, rc2, "second pass (%d reads): %s", (int)picked.size(), ctx->child ? ctx->child->err.c_str() : "");
  // ---- merge: the job slots of the second pass's reads from its result, every other slot from the first pass's
  hipStream_t st = ctx->stream;
  const int na = out->num_aln, R = n_reads, R2 = (int)picked.size();
  if (o2.num_aln != na) return lra_set_err(ctx, LRA_ERR_INVALID, "passes disagree on NumAln");
  const uint64_t S = (uint64_t)R * na;
  std::vector<int32_t> inB((size_t)R, -1);
  for (int i = 0; i < R2; i++) inB[picked[i]] = (int32_t)picked[i];    // (the second pass keeps the batch's slot numbering)
  int32_t* d_inB = (int32_t*)lra_ensure(ctx, 173, ((size_t)R + 4) * 4);
  uint64_t* d_src = (uint64_t*)lra_ensure(ctx, 175, (S + 4) * 8);
  if (!d_inB || !d_src) return LRA_ERR_NOMEM;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(d_inB, inB.data(), (size_t)R * 4, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_src_slot, grid(S), dim3(256), 0, st, S, na, (const int32_t*)d_inB, d_src);
  const lra_map_result a = *out;
  lra_merge::PassView A = lra_merge::view_of(a), B = lra_merge::view_of(o2);
  char* extra = nullptr;
  lra_map_result mo; memset(&mo, 0, sizeof mo);
  if ((rc = lra_merge::merge_passes(ctx, 171, S, na, d_src, A, B, a.n_alignments + o2.n_alignments, a.n_blocks + o2.n_blocks, a.n_runs + o2.n_runs,
                                    lra_merge::al256(S + 64) + ((size_t)R + 4) * 4, &extra, &mo))) return rc;
  uint8_t* reached = (uint8_t*)extra; uint32_t* rstat = (uint32_t*)(extra + lra_merge::al256(S + 64));
  hipLaunchKernelGGL(k_merge_reached, grid(S), dim3(256), 0, st, S, (const uint64_t*)d_src, a.d_job_reached, o2.d_job_reached, reached);
  hipLaunchKernelGGL(k_merge_read_status, grid(R), dim3(256), 0, st, R, (const int32_t*)d_inB, a.d_read_status, o2.d_read_status, rstat);
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));                          // (inB is pageable; and the result is the caller's to read now)
  LRA_HIP_CHECK(ctx, hipGetLastError());
  *out = mo;
  out->n_reads = R; out->num_aln = na; out->d_job_reached = reached; out->d_read_status = rstat; out->d_strands = a.d_strands; out->rc_base = a.rc_base;
  // counters: the stages up to the split point saw every read in the first pass; the later ones saw each read in one pass only
  lra_map_counters c = a.counters; const lra_map_counters& b = o2.counters;
  c.n_merged_clusters += b.n_merged_clusters; c.n_sdp2_anchors += b.n_sdp2_anchors; c.n_sdp2_entries += b.n_sdp2_entries; c.n_a13_blocks += b.n_a13_blocks;
  c.n_large_spaces += b.n_large_spaces; c.n_segments += b.n_segments; c.n_rows += b.n_rows; c.n_cells += b.n_cells; c.n_aog += b.n_aog;
  c.n_deferred_reads = a.counters.n_deferred_reads + (uint64_t)R2;
  out->counters = c;
  return LRA_OK;
}

// ---- two-stage batches: a batch's front half (a1 .. the second LinearExtend) on the context, its back half (second sparse DP .. statistics) on the companion
// context, so that batch i + 1's front half runs BESIDE batch i's back half (two host threads).  The front half is short wide kernels and rounds of small latency-bound
// launches, the back half is the sparse DP over the merged clusters and the banded refinement: side by side each fills what the other leaves idle.
static int front_checks(lra_ctx* ctx, int n_reads, const lra_map_opts* o) {
  if (!ctx || !o || n_reads < 0) return LRA_ERR_INVALID;
  { int rc = lra_map_ready(ctx, o, true); if (rc) return rc; }
  if (o->defer_matches > 0 || o->defer_seed_matches > 0) return lra_set_err(ctx, LRA_ERR_INVALID, "two-stage batches do not combine with defer_matches / defer_seed_matches");
  return LRA_OK;
}
// A front half that fails still hands over a batch -- an error batch: the back call that takes it returns the front half's code and holds nothing, so the
// thread that runs the back halves is never left waiting for a batch that will not come (one back call per front call, whatever the front call returned).
static int front_failed(lra_ctx* ctx, lra_handover* H, int rc) {
  const std::string msg = ctx->err;
  { std::unique_lock<std::mutex> lk(H->mu); H->cv.wait(lk, [&] { return !H->pending; }); H->in = LowaccTailIn(); H->in.n_reads = 0; H->rc = rc; H->err = msg; H->pending = true; }
  H->cv.notify_all();
  return rc;
}
// the back context and the two handover contexts (b -> hand[0] -> hand[1] on the child chain: destroyed with the context, timed with it); made once, by the first front call
static int two_stage_contexts(lra_ctx* ctx, lra_handover* H) {
  if (!ctx->child) { int rc = ensure_child(ctx, false); if (rc) return rc; }
  {
    // A companion the one call's second pass made earlier (defer_matches: lowest priority, the one call's tuning) becomes the back context: the back half's priority
    // and the choices made for device time, whoever made it.
    lra_ctx* c = ctx->child;
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    int want = getenv("LRA_BACK_PRIORITY") ? atoi(getenv("LRA_BACK_PRIORITY")) : greatest;
    want = std::max(greatest, std::min(least, want));
    if (c->owns_stream && c->stream && c->prio != want && !H->hand[0]) {     // (only before the first two-stage batch: nothing of a pipeline runs on it yet)
      LRA_HIP_CHECK(ctx, hipStreamSynchronize(c->stream));
      hipStream_t ns = nullptr;
      if (hipStreamCreateWithPriority(&ns, hipStreamNonBlocking, want) != hipSuccess) return lra_set_err(ctx, LRA_ERR_HIP, "companion stream");
      (void)hipStreamDestroy(c->stream);
      c->stream = ns; c->prio = want;
    }
    c->pipelined = true;
  }
  lra_ctx* tail = ctx->child;
  for (int i = 0; i < 2; i++) {
    if (!H->hand[i]) {
      if (tail->child) return lra_set_err(ctx, LRA_ERR_INVALID, "the companion context already has a companion of its own");
      lra_ctx* c = nullptr;
      int rc = lra_ctx_create(ctx->device, &c);
      if (rc) return lra_set_err(ctx, rc, "handover context");
      c->timing = ctx->timing;
      tail->child = c; H->hand[i] = c;
    }
    tail = H->hand[i];
  }
  return LRA_OK;
}
extern "C" int lra_map_reads_lowacc_front(lra_ctx* ctx, int n_reads, const char* d_seq, const uint64_t* d_read_off, uint64_t total_bases, const lra_map_opts* o) {
  if (!ctx) return LRA_ERR_INVALID;
  lra_handover* H = handover_of(ctx);
  { int rc = front_checks(ctx, n_reads, o); if (rc) return front_failed(ctx, H, rc); }
  { int rc = two_stage_contexts(ctx, H); if (rc) return front_failed(ctx, H, rc); }
  ctx->pipelined = true;
  if (n_reads == 0) {                                                     // an empty batch still takes its turn
    { std::unique_lock<std::mutex> lk(H->mu); H->cv.wait(lk, [&] { return !H->pending; }); H->in = LowaccTailIn(); H->in.n_reads = 0; H->rc = LRA_OK; H->pending = true; }
    H->cv.notify_all();
    return LRA_OK;
  }
  lra_map_result tmp;
  const std::function<int()> none;
  const int rc = lowacc_core(ctx, n_reads, d_seq, d_read_off, total_bases, o, &tmp, 0, nullptr, nullptr, nullptr, none, H);
  return rc ? front_failed(ctx, H, rc) : LRA_OK;                         // (lowacc_core hands the batch over as its last act: a failure means it has not)
}
extern "C" int lra_map_reads_lowacc_back(lra_ctx* ctx, const lra_map_opts* o, lra_map_result* out, lra_ctx** back_ctx) {
  if (!ctx || !o || !out) return LRA_ERR_INVALID;
  lra_handover* H = handover_of(ctx);
  LowaccTailIn in;
  int frc = LRA_OK; std::string ferr;
  const double tw0 = lra_wall_ms();
  {                                                                      // (waits for a front half, however long; a front half that fails hands over an error batch)
    std::unique_lock<std::mutex> lk(H->mu);
    if (H->busy) return lra_set_err(ctx->child ? ctx->child : ctx, LRA_ERR_INVALID, "the result of the back half before this one is still held (lra_map_back_release)");
    H->cv.wait(lk, [&] { return H->pending; });
    in = H->in; frc = H->rc; ferr = H->err; H->rc = LRA_OK; H->err.clear();
    H->pending = false;
    H->busy = frc == LRA_OK;                                             // an error batch holds nothing
  }
  H->cv.notify_all();                                                    // (the front half may hand over the next batch now)
  if (getenv("LRA_TWO_STAGE_DBG")) fprintf(stderr, "[two-stage] back half waited %.0f ms for a front half\n", lra_wall_ms() - tw0);
  memset(out, 0, sizeof *out);
  lra_ctx* b = ctx->child;                                               // (made by the first front half)
  if (back_ctx) *back_ctx = b;
  // (this thread's error text goes to the BACK context -- the front thread writes ctx's; without a back context the front half has failed before making one, and is not running)
  if (frc) return lra_set_err(b ? b : ctx, frc, "front half of this batch failed: %s", ferr.c_str());
  // The back context's view of the reference data (borrowed from ctx), refreshed here -- by the thread that owns the back context, with nothing running on it.
  // (Reloading ctx's reference is for when no batch is in flight: the halves of the batches in flight read it.)
  int rc = child_refresh(ctx);
  if (rc == LRA_OK) {
    b->map->last_text.clear(); b->map->last_sig = lra_map_sig{};
    out->n_reads = in.n_reads;
    if (in.n_reads == 0) return LRA_OK;
    rc = lowacc_tail(b, in, o, out);
  }
  if (rc == LRA_OK) rc = lra_map_count_flagged(b, out);
  if (rc) { const std::string msg = b->err; return lra_set_err(b, rc, "back half: %s", msg.c_str()); }
  return LRA_OK;
}
extern "C" int lra_map_back_release(lra_ctx* ctx) {
  if (!ctx || !ctx->handover) return LRA_ERR_INVALID;
  lra_handover* H = ctx->handover;
  { std::lock_guard<std::mutex> lk(H->mu); if (!H->busy) return lra_set_err(ctx->child ? ctx->child : ctx, LRA_ERR_INVALID, "no back half's result is held"); H->busy = false; }
  H->cv.notify_all();
  return LRA_OK;
}

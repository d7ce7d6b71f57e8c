// lra_amd/csrc/map_common.hip -- the stages MapRead_lowacc (mapread.hip) and MapRead_highacc (mapread_highacc.hip) run the same way, once (gfx950 only):
// whether a batch may be mapped, its seed result, the forward + reverse-complement read buffer, tinyOpts, every SegAlignment addressed and through
// IndelRefineAlignment, RefineBreakpoint, the result as the caller sees it, and the stage timer.  Declared in map_state.h.
#include "common.h"
#include "seed_state.h"
#include "scan.h"
#include "map_state.h"
#include <chrono>
#include <stdlib.h>
#include <algorithm>
#include <vector>

namespace {

__global__ void k_add_off(int n, const uint64_t* __restrict__ off, uint64_t add, uint64_t* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= n) out[i] = off[i];                       // [0..n]: the reads forward
  if (i >= 1 && i <= n) out[n + i] = off[i] + add;   // [n+1..2n]: their reverse complements
}

// per alignment: which read, where its strand's bases start, where its chromosome starts and how long it is
__global__ void k_aln_address(uint64_t n_jobs, int num_aln, const uint64_t* __restrict__ job_aln_off, const int32_t* __restrict__ strand,
                              const int32_t* __restrict__ chrom, const uint64_t* __restrict__ read_off, uint64_t rc_base,
                              const uint64_t* __restrict__ chrom_pos, uint32_t* __restrict__ aln_read, uint64_t* __restrict__ q_off,
                              int32_t* __restrict__ q_len, uint64_t* __restrict__ t_off, int64_t* __restrict__ t_len) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_jobs) return;
  const uint32_t r = (uint32_t)(j / (uint64_t)num_aln);
  for (uint64_t a = job_aln_off[j]; a < job_aln_off[j + 1]; a++) {
    aln_read[a] = r;
    q_off[a] = read_off[r] + (strand[a] ? rc_base : 0);
    q_len[a] = (int32_t)(read_off[r + 1] - read_off[r]);
    const int c = chrom[a];
    t_off[a] = chrom_pos[c];
    t_len[a] = (int64_t)(chrom_pos[c + 1] - chrom_pos[c]);
  }
}

// ---- RefineBreakpoint between consecutive SegAlignments of a job (Map_lowacc.h:586-596), one round per junction index
__global__ void k_bp_params(int n, const uint32_t* __restrict__ jl, const uint32_t* __restrict__ jr, const uint64_t* __restrict__ boff,
                            const int32_t* __restrict__ strand, const uint64_t* __restrict__ q_off, const int32_t* __restrict__ q_len,
                            const uint64_t* __restrict__ t_off, const int64_t* __restrict__ t_len, uint32_t* l_cnt, uint32_t* r_cnt, int32_t* read_len,
                            int32_t* l_strand, uint64_t* l_read, uint64_t* l_coff, int32_t* l_clen, int32_t* r_strand, uint64_t* r_read, uint64_t* r_coff,
                            int32_t* r_clen) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t a = jl[j], b = jr[j];
  l_cnt[j] = (uint32_t)(boff[a + 1] - boff[a]); r_cnt[j] = (uint32_t)(boff[b + 1] - boff[b]);
  read_len[j] = q_len[a];
  l_strand[j] = strand[a]; l_read[j] = q_off[a]; l_coff[j] = t_off[a]; l_clen[j] = (int32_t)t_len[a];
  r_strand[j] = strand[b]; r_read[j] = q_off[b]; r_coff[j] = t_off[b]; r_clen[j] = (int32_t)t_len[b];
}
__global__ void __launch_bounds__(64) k_bp_gather(int n, const uint32_t* __restrict__ jl, const uint32_t* __restrict__ jr, const uint64_t* __restrict__ boff,
                                                  const int32_t* __restrict__ blocks, const uint64_t* __restrict__ l_off, const uint64_t* __restrict__ r_off,
                                                  int32_t* l_blocks, int32_t* r_blocks) {
  const int j = blockIdx.x >> 1, side = blockIdx.x & 1;
  if (j >= n) return;
  const uint32_t a = side ? jr[j] : jl[j];
  const int32_t* s = blocks + 3 * boff[a];
  int32_t* d = side ? r_blocks + 3 * r_off[j] : l_blocks + 3 * l_off[j];
  const uint64_t w = 3 * (boff[a + 1] - boff[a]);
  for (uint64_t x = threadIdx.x; x < w; x += 64) d[x] = s[x];
}
__global__ void k_bp_counts(uint64_t nA, const uint64_t* __restrict__ boff, uint32_t* cnt, int32_t* touched) {
  const uint64_t a = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= nA) return;
  cnt[a] = (uint32_t)(boff[a + 1] - boff[a]); touched[a] = -1;
}
__global__ void k_bp_touch(int n, const uint32_t* __restrict__ jl, const uint32_t* __restrict__ jr, const int32_t* __restrict__ l_n, const int32_t* __restrict__ r_n,
                           uint32_t* cnt, int32_t* touched) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  cnt[jl[j]] = (uint32_t)l_n[j]; touched[jl[j]] = 2 * j;
  cnt[jr[j]] = (uint32_t)r_n[j]; touched[jr[j]] = 2 * j + 1;
}
__global__ void __launch_bounds__(64) k_bp_scatter(uint64_t nA, const uint64_t* __restrict__ old_off, const int32_t* __restrict__ old_blocks,
                                                   const uint64_t* __restrict__ new_off, const int32_t* __restrict__ touched, const int32_t* __restrict__ l_blocks,
                                                   const uint64_t* __restrict__ l_off, const int32_t* __restrict__ r_blocks, const uint64_t* __restrict__ r_off,
                                                   int32_t* new_blocks) {
  const uint64_t a = blockIdx.x;
  if (a >= nA) return;
  const int32_t tch = touched[a];
  const int32_t* s = tch < 0 ? old_blocks + 3 * old_off[a] : (tch & 1) ? r_blocks + 3 * r_off[tch >> 1] : l_blocks + 3 * l_off[tch >> 1];
  int32_t* d = new_blocks + 3 * new_off[a];
  const uint64_t w = 3 * (new_off[a + 1] - new_off[a]);
  for (uint64_t x = threadIdx.x; x < w; x += 64) d[x] = s[x];
}

}  // namespace

// RefineBreakpoint(read, genome, *SegAlignment[s], *SegAlignment[s-1], opts) for s = 1, 2, ... of every job: round k runs junction k of all
// jobs that have one (segment k is "left", segment k - 1 -- already refined against k - 2 in the round before -- is "right").
int lra_refine_breakpoints(lra_ctx* ctx, uint64_t nJ, uint64_t nA, const uint64_t* d_job_aln_off, const int32_t* d_strand, const uint64_t* q_off, const int32_t* q_len,
                              const uint64_t* t_off, const int64_t* t_len, const char* strands, const char* genome, lra_refine_result* fres) {
  hipStream_t st = ctx->stream;
  std::vector<uint64_t> jo(nJ + 1);
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(jo.data(), d_job_aln_off, (nJ + 1) * 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  uint64_t max_seg = 0;
  for (uint64_t j = 0; j < nJ; j++) max_seg = std::max(max_seg, jo[j + 1] - jo[j]);
  const int32_t* cur_blocks = fres->d_blocks; const uint64_t* cur_off = fres->d_block_off;
  uint64_t n_blocks = fres->n_blocks;
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  for (uint64_t k = 1; k < max_seg; k++) {
    std::vector<uint32_t> hl, hr;
    for (uint64_t j = 0; j < nJ; j++) if (jo[j + 1] - jo[j] > k) { hl.push_back((uint32_t)(jo[j] + k)); hr.push_back((uint32_t)(jo[j] + k - 1)); }
    const int n = (int)hl.size();
    if (!n) break;
    const size_t n1 = (size_t)n + 2;
    char* w = (char*)lra_ensure(ctx, 72, al(n1 * 4) * 9 + al(n1 * 8) * 6 + al((nA + 2) * 4) * 2 + al((nA + 2) * 8) + 4096);
    if (!w) return LRA_ERR_NOMEM;
    auto take = [&](size_t bytes) { char* r = w; w += al(bytes); return r; };
    uint32_t* jl = (uint32_t*)take(n1 * 4); uint32_t* jr = (uint32_t*)take(n1 * 4); uint32_t* l_cnt = (uint32_t*)take(n1 * 4); uint32_t* r_cnt = (uint32_t*)take(n1 * 4);
    int32_t* read_len = (int32_t*)take(n1 * 4); int32_t* l_strand = (int32_t*)take(n1 * 4); int32_t* r_strand = (int32_t*)take(n1 * 4);
    int32_t* l_clen = (int32_t*)take(n1 * 4); int32_t* r_clen = (int32_t*)take(n1 * 4);
    uint64_t* l_read = (uint64_t*)take(n1 * 8); uint64_t* r_read = (uint64_t*)take(n1 * 8); uint64_t* l_coff = (uint64_t*)take(n1 * 8); uint64_t* r_coff = (uint64_t*)take(n1 * 8);
    uint64_t* l_off = (uint64_t*)take(n1 * 8); uint64_t* r_off = (uint64_t*)take(n1 * 8);
    uint32_t* cnt = (uint32_t*)take((nA + 2) * 4); int32_t* touched = (int32_t*)take((nA + 2) * 4); uint64_t* new_off_tmp = (uint64_t*)take((nA + 2) * 8);
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(jl, hl.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(jr, hr.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_bp_params, dim3((n + 255) / 256), dim3(256), 0, st, n, jl, jr, cur_off, d_strand, q_off, q_len, t_off, t_len, l_cnt, r_cnt, read_len, l_strand,
                       l_read, l_coff, l_clen, r_strand, r_read, r_coff, r_clen);
    int rc;
    if ((rc = lra_exclusive_scan<uint32_t>(ctx, n, l_cnt, l_off)) || (rc = lra_exclusive_scan<uint32_t>(ctx, n, r_cnt, r_off))) return rc;
    uint64_t tl = 0, tr = 0;
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&tl, l_off + n, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&tr, r_off + n, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    int32_t* lb = (int32_t*)lra_ensure(ctx, 73, al((tl + 1) * 12) + al((tr + 1) * 12) + 512);
    if (!lb) return LRA_ERR_NOMEM;
    int32_t* rb = (int32_t*)((char*)lb + al((tl + 1) * 12));
    hipLaunchKernelGGL(k_bp_gather, dim3(2 * n), dim3(64), 0, st, n, jl, jr, cur_off, cur_blocks, l_off, r_off, lb, rb);
    lra_breakpoint_result br;
    if ((rc = lra_refine_breakpoint_batch(ctx, n, read_len, strands, genome, lb, l_off, l_strand, l_read, l_coff, l_clen, rb, r_off, r_strand, r_read, r_coff, r_clen, &br)))
      return rc;
    hipLaunchKernelGGL(k_bp_counts, dim3((unsigned)((nA + 255) / 256)), dim3(256), 0, st, nA, cur_off, cnt, touched);
    hipLaunchKernelGGL(k_bp_touch, dim3((n + 255) / 256), dim3(256), 0, st, n, jl, jr, br.d_l_n, br.d_r_n, cnt, touched);
    if ((rc = lra_exclusive_scan<uint32_t>(ctx, (long)nA, cnt, new_off_tmp))) return rc;
    uint64_t nb = 0;
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&nb, new_off_tmp + nA, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    const int slot = 74 + (int)(k & 1);                                   // ping-pong: the other slot may hold the current blocks
    char* nbuf = (char*)lra_ensure(ctx, slot, al((nb + 1) * 12) + al((nA + 2) * 8) + 512);
    if (!nbuf) return LRA_ERR_NOMEM;
    int32_t* new_blocks = (int32_t*)nbuf; uint64_t* new_off = (uint64_t*)(nbuf + al((nb + 1) * 12));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(new_off, new_off_tmp, (nA + 1) * 8, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_bp_scatter, dim3((unsigned)nA), dim3(64), 0, st, nA, cur_off, cur_blocks, new_off, touched, br.d_l_blocks, br.d_l_off, br.d_r_blocks, br.d_r_off,
                       new_blocks);
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    cur_blocks = new_blocks; cur_off = new_off; n_blocks = nb;
  }
  fres->d_blocks = cur_blocks; fres->d_block_off = cur_off; fres->n_blocks = n_blocks;
  return LRA_OK;
}

int lra_map_ready(lra_ctx* ctx, const lra_map_opts* o, bool gli_required) {
  const lra_map_state* m = ctx->map;
  if (!m || (gli_required ? !m->gli_buf : m->chrom_pos.size() < 2) || !ctx->seed || !ctx->seed->genome || !ctx->seed->idx_key)
    return lra_set_err(ctx, LRA_ERR_INVALID, gli_required ? "reference not loaded (genome, global index, chromosome table, local index)"
                                                          : "reference not loaded (genome, global index, chromosome table)");
  if (m->gli_buf && (m->gli_window != o->localIndexWindow || m->gli_k != o->localK || m->gli_w != o->localW))    // (whether or not a read of this batch takes a branch that reads glIndex)
    return lra_set_err(ctx, LRA_ERR_INVALID, "the genome's local index has k = %d, w = %d, windows of %d bases; the options say %d, %d, %d (lra_map_opts_apply_local_index: glIndex.Read overrides them)",
                       m->gli_k, m->gli_w, m->gli_window, o->localK, o->localW, o->localIndexWindow);
  return lra_map_check_shared(ctx);
}

int lra_map_seed(lra_ctx* ctx, int n_reads, const char* d_seq, const uint64_t* d_read_off, int K, int W, int max_freq, uint32_t defer_T, lra_seed_result* sres) {
  // (lra align -a, lra_ctx_set_store_all: the sketch alone takes w = 1, MapRead.h:172-176; the stages behind it keep the caller's W)
  const int seedW = ctx->store_all ? 1 : W;
  // (a result made ahead of the call from these reads with these parameters is what lra_seed_batch would make)
  const bool ahead = ctx->ahead.valid && ctx->ahead.n_reads == n_reads && ctx->ahead.d_seq == d_seq && ctx->ahead.d_read_off == d_read_off &&
                     ctx->ahead.k == K && ctx->ahead.w == seedW && ctx->ahead.max_freq == max_freq;
  ctx->ahead.valid = false;
  if (ahead) {
    if (defer_T) return lra_set_err(ctx, LRA_ERR_INVALID, "defer_seed_matches and a seed result adopted ahead of the call do not combine");
    *sres = ctx->ahead.res;
    return LRA_OK;
  }
  ctx->seed->defer_T = defer_T;
  const int rc = lra_seed_batch(ctx, n_reads, d_seq, d_read_off, K, seedW, max_freq, sres);
  ctx->seed->defer_T = 0;
  return rc;
}

int lra_map_strands(lra_ctx* ctx, int n_reads, const char* d_seq, const uint64_t* d_read_off, uint64_t tot, char** both_out) {
  hipStream_t st = ctx->stream;
  char* both = (char*)lra_ensure(ctx, 57, lra_strands_bytes(tot, n_reads));
  if (!both) return LRA_ERR_NOMEM;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(both, d_seq, tot, hipMemcpyDeviceToDevice, st));
  LRA_HIP_CHECK(ctx, hipMemsetAsync(both + 2 * tot, 0, 64, st));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(both + lra_strands_ro_at(tot), d_read_off, ((size_t)n_reads + 1) * 8, hipMemcpyDeviceToDevice, st));
  *both_out = both;
  return lra_create_rc_batch(ctx, n_reads, d_seq, d_read_off, both + tot);
}

uint64_t* lra_map_strand_offsets(lra_ctx* ctx, int n_reads, const uint64_t* d_read_off, uint64_t tot) {
  uint64_t* off2 = (uint64_t*)lra_ensure(ctx, 58, (2 * (size_t)n_reads + 2) * 8);
  if (off2) hipLaunchKernelGGL(k_add_off, dim3((n_reads + 256) / 256), dim3(256), 0, ctx->stream, n_reads, d_read_off, tot, off2);
  return off2;
}

lra_lra_opts lra_map_lra_opts(const lra_map_opts* o) {
  lra_lra_opts lo; lo.localW = o->localW; lo.globalW = o->localW; lo.localMaxFreq = o->localMaxFreq; lo.match = o->localMatch; lo.mismatch = o->localMismatch;
  lo.indel = o->localIndel; lo.localBand = o->localBand; lo.refineBySDP = 1; lo.isOnt = (o->readType == LRA_READ_ONT || o->readType == LRA_READ_CLR) ? 1 : 0;
  lo.gapopen = o->sdp.gapopen; lo.gapextend = o->sdp.gapextend; lo.gaproot = o->sdp.gaproot; lo.gapCeiling1 = o->sdp.gapCeiling1; lo.gapCeiling2 = o->sdp.gapCeiling2;
  return lo;
}

int lra_map_finish_alignments(lra_ctx* ctx, const lra_map_opts* o, int num_aln, uint64_t n_jobs, const lra_alignments_result* ares, const uint64_t* d_read_off,
                              const char* both, uint64_t tot, int endAlign, lra_map_finish* f) {
  hipStream_t st = ctx->stream;
  const uint64_t nA = ares->n_alignments;
  f->aln_read = (uint32_t*)lra_ensure(ctx, 59, (nA + 1) * 4);
  f->q_off = (uint64_t*)lra_ensure(ctx, 60, (nA + 1) * 8);
  f->q_len = (int32_t*)lra_ensure(ctx, 61, (nA + 1) * 4);
  f->t_off = (uint64_t*)lra_ensure(ctx, 62, (nA + 1) * 8);
  f->t_len = (int64_t*)lra_ensure(ctx, 63, (nA + 1) * 8);
  if (!f->aln_read || !f->q_off || !f->q_len || !f->t_off || !f->t_len) return LRA_ERR_NOMEM;
  if (n_jobs) hipLaunchKernelGGL(k_aln_address, grid(n_jobs), dim3(256), 0, st, n_jobs, num_aln, ares->d_job_aln_off, ares->d_strand, ares->d_chrom, d_read_off, tot,
                                 (const uint64_t*)ctx->map->d_chrom_pos, f->aln_read, f->q_off, f->q_len, f->t_off, f->t_len);
  lra_refine_result& fres = f->fres;
  memset(&fres, 0, sizeof fres);
  if (!nA) return LRA_OK;
  int rc;
  if (o->skipBandedRefine) {
    fres.n_aln = (int)nA; fres.n_blocks = ares->n_blocks; fres.d_block_off = ares->d_block_off; fres.d_blocks = ares->d_blocks; fres.d_status = nullptr;
  } else if ((rc = lra_indel_refine_batch(ctx, (int)nA, ares->d_blocks, ares->d_block_off, ares->n_blocks, both, f->q_off, f->q_len, (const char*)ctx->seed->genome, f->t_off,
                                          f->t_len, o->refineBand, o->localMatch, o->localMismatch, o->localIndel, endAlign, &fres))) return rc;
  if (fres.d_status) {                                                    // the refine stage's status array lives in scratch the next stage reuses
    int32_t* keep = (int32_t*)lra_ensure(ctx, 64, (nA + 1) * 4);
    if (!keep) return LRA_ERR_NOMEM;
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(keep, fres.d_status, nA * 4, hipMemcpyDeviceToDevice, st));
    fres.d_status = keep;
  }
  return LRA_OK;
}

void lra_map_fill_result(lra_map_result* out, int num_aln, uint64_t n_jobs, const lra_alignments_result& ares, const lra_map_finish& f, const lra_stats_result& tres,
                         const char* both, uint64_t tot, uint8_t* job_reached, uint32_t* read_status) {
  const lra_refine_result& fres = f.fres;
  out->num_aln = num_aln; out->n_jobs = n_jobs; out->n_alignments = ares.n_alignments; out->n_blocks = fres.n_blocks; out->n_runs = tres.n_runs;
  out->d_job_aln_off = ares.d_job_aln_off; out->d_job_status = ares.d_status; out->d_job_reached = job_reached; out->d_read_status = read_status;
  out->d_aln_read = f.aln_read; out->d_strand = ares.d_strand; out->d_supp = ares.d_supp; out->d_secondary = ares.d_secondary; out->d_n0 = ares.d_n0; out->d_n1 = ares.d_n1;
  out->d_chrom = ares.d_chrom; out->d_first_sdp_value = ares.d_value;
  out->d_block_off = fres.d_block_off; out->d_blocks = fres.d_blocks; out->d_refine_status = fres.d_status;
  out->d_counts = tres.d_counts; out->d_value = tres.d_value; out->d_run_off = tres.d_run_off; out->d_runs = tres.d_runs;
  out->d_strands = both; out->rc_base = tot;
}

double lra_wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
lra_stage_timer::lra_stage_timer(lra_ctx* c) : ctx(c), on(getenv("LRA_STAGE_DBG") != nullptr) { (*this)(nullptr); }
void lra_stage_timer::operator()(const char* name) {                      // (name == nullptr: start the clock)
  if (!on) return;
  (void)hipStreamSynchronize(ctx->stream);
  const double t = lra_wall_ms();
  if (name) fprintf(stderr, "[stage%s] %-28s %8.1f ms\n", ctx->owns_stream ? " 2nd" : "", name, t - t_prev);
  t_prev = t;
}

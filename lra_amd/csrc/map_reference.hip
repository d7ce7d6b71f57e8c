// lra_amd/csrc/map_reference.hip -- the reference data the two drivers map against, per context: the chromosome table, the genome's local index (built
// on the device or handed over from a .gli file), sharing one replica between contexts, and the four presets of lra_map_opts with what glIndex.Read
// leaves in their place (gfx950 only).
#include "common.h"
#include "seed_state.h"
#include "map_state.h"
#include <math.h>
#include <stdlib.h>
#include <algorithm>

void lra_map_free(lra_ctx* ctx) {
  lra_map_state* m = ctx->map;
  if (!m) return;
  if (!m->borrowed) {
    m->cell->dead = true;                                                  // borrowers hold the cell, not this state
    if (m->d_chrom_pos) (void)hipFree(m->d_chrom_pos);
    if (m->gli_buf) (void)hipFree(m->gli_buf);
    if (m->d_gso) (void)hipFree(m->d_gso);
  }
  delete m;
  ctx->map = nullptr;
}

namespace {

lra_map_state* map_state(lra_ctx* ctx) {
  if (!ctx->map) ctx->map = new lra_map_state();
  return ctx->map;
}

// a loader on a context that borrows its reference data: drop the owner's pointers, own what is loaded from here on
void map_disown(lra_map_state* m) {
  if (!m->borrowed) return;
  m->d_chrom_pos = nullptr; m->gli_buf = nullptr; m->gli = lra_local_index_result{}; m->d_gso = nullptr; m->n_gwin = 0; m->gli_window = 0;
  m->borrowed = false; m->owner_cell.reset(); m->owner_generation = 0;
}

}  // namespace

extern "C" void lra_map_opts_preset_ont(lra_map_opts* o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  // -ONT (lra.cpp:386-431) over the defaults of Options.h:127-230
  o->globalK = 17; o->globalW = 10; o->globalMaxFreq = 150;
  o->localK = 10; o->localW = 5; o->localMaxFreq = 15; o->localIndexWindow = 256;
  o->refineBand = 7; o->localMatch = 4; o->localMismatch = -1; o->localIndel = -2; o->localBand = 15;
  o->refineSpaceDist = 30000; o->anchorstoosparse = 0.005f; o->splitdist = 50000; o->window = 100;
  o->second_anchorbonus = 2.0f; o->bypassClustering = 1; o->skipBandedRefine = 0;
  o->clean.globalK = 17; o->clean.cleanMaxDiag = 200; o->clean.minDiagCluster = 3; o->clean.bypassClustering = 1; o->clean.cleanClustersize = 100;
  o->clean.SecondCleanMinDiagCluster = 10; o->clean.SecondCleanMaxDiag = 100; o->clean.punish_anchorfreq = 5; o->clean.anchorPerlength = 5;
  o->sdp.rate = 20.0f; o->sdp.NumAln = 2; o->sdp.alnthres = 0.65f; o->sdp.gapopen = 7.0f; o->sdp.gapextend = 10.0f; o->sdp.gaproot = 1.5f;
  o->sdp.gapCeiling1 = 1500; o->sdp.gapCeiling2 = 3000; o->sdp.mode = 0; o->sdp.globalK = 17;
  o->readType = LRA_READ_ONT; o->hardClip = 1; o->PrintNumAln = 1; o->printFormat = 's';
  o->flagged_unaligned = 0;    // a flagged read gets an empty record (the caller re-runs it; counters.n_flagged_reads)
  o->defer_matches = 0;        // one pass (lra_map_reads_lowacc_batch: the second, concurrent pass is built and tested, and measured to be no gain on this device)
}

extern "C" void lra_map_opts_preset_clr(lra_map_opts* o) {
  if (!o) return;
  lra_map_opts_preset_ont(o);
  // -CLR (lra.cpp:341-386): what differs from -ONT on this path
  o->globalK = 15; o->globalMaxFreq = 250; o->refineBand = 20; o->second_anchorbonus = 6.0f;
  o->clean.globalK = 15; o->clean.SecondCleanMaxDiag = 120;
  o->sdp.rate = 15.0f; o->sdp.alnthres = 0.50f; o->sdp.globalK = 15;
  o->readType = LRA_READ_CLR;
}

extern "C" void lra_map_opts_preset_ccs(lra_map_opts* o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  // -CCS (lra.cpp:306-340) over the defaults of Options.h:127-230.  globalK: the preset says 25, but `lra align` then reads the index file, and ReadIndex
  // overwrites opts.globalK with the K the index was built with (MMIndex.h:409, lra.cpp:623) -- 17 for `lra index -CCS` (lra.cpp:890-896); globalW stays 20.
  o->globalK = 17; o->globalW = 20; o->globalMaxFreq = 150;
  o->localK = 7; o->localW = 5; o->localMaxFreq = 15; o->localIndexWindow = 256;
  o->refineBand = 7; o->localMatch = 4; o->localMismatch = -3; o->localIndel = -4; o->localBand = 15;
  o->refineSpaceDist = 30000; o->anchorstoosparse = 0.005f; o->splitdist = 50000; o->window = 100;
  o->second_anchorbonus = 2.0f; o->bypassClustering = 0; o->skipBandedRefine = 0; o->refineBreakpoint = 0;
  o->clean.globalK = 17; o->clean.cleanMaxDiag = 150; o->clean.minDiagCluster = 10; o->clean.bypassClustering = 0; o->clean.cleanClustersize = 100;
  o->clean.SecondCleanMinDiagCluster = 30; o->clean.SecondCleanMaxDiag = 100; o->clean.punish_anchorfreq = 10; o->clean.anchorPerlength = 10;
  o->sdp.rate = 10.0f; o->sdp.NumAln = 2; o->sdp.alnthres = 0.7f; o->sdp.gapopen = 4.0f; o->sdp.gapextend = 15.0f; o->sdp.gaproot = 1.5f;
  o->sdp.gapCeiling1 = 2000; o->sdp.gapCeiling2 = 3000; o->sdp.mode = 0; o->sdp.globalK = 17;
  o->readType = LRA_READ_CCS; o->hardClip = 1; o->PrintNumAln = 1; o->printFormat = 's';
  o->fine.globalK = 17; o->fine.RoughClustermaxGap = 500; o->fine.maxDiag = 500; o->fine.maxGap = 400; o->fine.minClusterSize = 10; o->fine.minUniqueStretchNum = 1;
  o->fine.minUniqueStretchDist = 50;
  o->merge_dist = 100;
}

extern "C" void lra_map_opts_preset_contig(lra_map_opts* o) {
  if (!o) return;
  lra_map_opts_preset_ccs(o);
  // -CONTIG (lra.cpp:268-305): what differs from -CCS on this path
  o->globalK = 19; o->globalW = 10; o->globalMaxFreq = 30; o->refineBand = 50; o->refineSpaceDist = 50000;
  o->clean.globalK = 19; o->clean.minDiagCluster = 30;
  o->sdp.rate = 1.0f; o->sdp.gapextend = 20.0f; o->sdp.gapCeiling1 = 3000; o->sdp.gapCeiling2 = 5000; o->sdp.globalK = 19;
  o->fine.globalK = 19; o->fine.maxDiag = 100; o->fine.maxGap = 500;
  o->readType = LRA_READ_CONTIG;
}

// What glIndex.Read leaves in the options' place (lra.cpp:627, MMIndex.h:154-173): the .gli file's k, w and localIndexWindow are the genome index's AND, through the copy
// constructor (MMIndex.h:128-136, Map_lowacc.h:246-247), the read indexes'; smallOpts.globalK / globalW are glIndex.k / w (Map_lowacc.h:233-234, Map_highacc.h:430-431).
// `lra index` writes k = 10, w = 5, windows of 2048 bases under every preset (LocalIndex(0): 1 << (LOCAL_POS_BITS - 1), MMIndex.h:110-127; RunStoreLocal, lra.cpp:778-850);
// without a .gli file `lra align` builds glIndex from opts.localK / localIndexWindow = 256 (lra.cpp:619-621, :628) -- the presets' values.
extern "C" void lra_map_opts_apply_local_index(lra_map_opts* o, int k, int w, int window) {
  if (!o) return;
  o->localK = k; o->localW = w; o->localIndexWindow = window;
}
extern "C" int lra_ctx_local_index_params(lra_ctx* ctx, int* k, int* w, int* window) {
  if (!ctx || !ctx->map || !ctx->map->gli_window) return LRA_ERR_INVALID;
  if (k) *k = ctx->map->gli_k;
  if (w) *w = ctx->map->gli_w;
  if (window) *window = ctx->map->gli_window;
  return LRA_OK;
}

extern "C" int lra_ctx_load_chromosomes(lra_ctx* ctx, const uint64_t* h_chrom_pos, int n_chrom) {
  if (!ctx || !h_chrom_pos || n_chrom < 1) return LRA_ERR_INVALID;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  lra_map_state* m = map_state(ctx);
  map_disown(m); m->cell->gen++;
  m->chrom_pos.assign(h_chrom_pos, h_chrom_pos + n_chrom + 1);
  if (m->d_chrom_pos) (void)hipFree(m->d_chrom_pos);
  LRA_HIP_CHECK(ctx, hipMalloc((void**)&m->d_chrom_pos, (size_t)(n_chrom + 1) * 8));
  LRA_HIP_CHECK(ctx, hipMemcpy(m->d_chrom_pos, h_chrom_pos, (size_t)(n_chrom + 1) * 8, hipMemcpyHostToDevice));
  if (m->lut.empty()) for (int i = 1; i < 10002; i += 5) m->lut.push_back(logf((float)i));   // LogLookUpTable.h:9-15
  return LRA_OK;
}

extern "C" int lra_ctx_build_local_index(lra_ctx* ctx, int k, int w, int window, int max_freq) {
  if (!ctx || !ctx->map || ctx->map->chrom_pos.size() < 2) return ctx ? lra_set_err(ctx, LRA_ERR_INVALID, "load the chromosome table first") : LRA_ERR_INVALID;
  if (!ctx->seed || !ctx->seed->genome) return lra_set_err(ctx, LRA_ERR_INVALID, "load the genome first");
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  lra_map_state* m = ctx->map;
  if (m->borrowed) return lra_set_err(ctx, LRA_ERR_INVALID, "this context shares another context's reference data: load its own chromosome table first");
  m->cell->gen++;
  const int n_chrom = (int)m->chrom_pos.size() - 1;
  if (m->chrom_pos[n_chrom] != ctx->seed->genome_len) return lra_set_err(ctx, LRA_ERR_INVALID, "chromosome table does not cover the genome");
  lra_local_index_result r;
  int rc = lra_local_index_batch(ctx, n_chrom, (const char*)ctx->seed->genome, m->d_chrom_pos, k, w, window, max_freq, &r);
  if (rc) return rc;
  // the result lives in a context buffer the reads' index will reuse: keep a copy
  if (m->gli_buf) (void)hipFree(m->gli_buf);
  LRA_HIP_CHECK(ctx, hipMalloc(&m->gli_buf, r.bytes + 256));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(m->gli_buf, r.d_base, r.bytes, hipMemcpyDeviceToDevice, ctx->stream));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  m->gli = r;
  const char* ob = (const char*)r.d_base; char* nb = (char*)m->gli_buf;
  m->gli.d_base = nb;
  m->gli.d_win_off = (const uint64_t*)(nb + ((const char*)r.d_win_off - ob));
  m->gli.d_tuple_bnd = (const uint64_t*)(nb + ((const char*)r.d_tuple_bnd - ob));
  m->gli.d_tuples = (const uint32_t*)(nb + ((const char*)r.d_tuples - ob));
  m->gli_window = window; m->gli_k = k; m->gli_w = w;
  // LocalIndex::seqOffsets (MMIndex.h:200-245): window ends, restarting at each sequence
  std::vector<uint64_t> gso; gso.push_back(0);
  for (int c = 0; c < n_chrom; c++)
    for (uint64_t p = m->chrom_pos[c]; p < m->chrom_pos[c + 1];) { p = std::min<uint64_t>(p + (uint64_t)window, m->chrom_pos[c + 1]); gso.push_back(p); }
  if (gso.size() != r.n_windows + 1) return lra_set_err(ctx, LRA_ERR_INVALID, "local index window count mismatch");
  if (m->d_gso) (void)hipFree(m->d_gso);
  LRA_HIP_CHECK(ctx, hipMalloc((void**)&m->d_gso, gso.size() * 8));
  LRA_HIP_CHECK(ctx, hipMemcpy(m->d_gso, gso.data(), gso.size() * 8, hipMemcpyHostToDevice));
  m->n_gwin = r.n_windows;
  return LRA_OK;
}

// glIndex as LocalIndex::Read left it (MMIndex.h:154-173): the .gli file's payload handed over as it is, instead of building the index again on the device.  The three
// arrays are copied; seq_offsets must be what IndexSeq writes for the loaded chromosome table and this window (MMIndex.h:200-245: window ends, restarting at every
// sequence) -- an index of another genome is refused.
extern "C" int lra_ctx_load_local_index(lra_ctx* ctx, int k, int w, int window, uint64_t n_windows, const uint64_t* h_seq_offsets, const uint64_t* h_tuple_bnd,
                                        uint64_t n_tuples, const uint32_t* h_tuples) {
  if (!ctx || !ctx->map || ctx->map->chrom_pos.size() < 2) return ctx ? lra_set_err(ctx, LRA_ERR_INVALID, "load the chromosome table first") : LRA_ERR_INVALID;
  if (!h_seq_offsets || !h_tuple_bnd || (n_tuples && !h_tuples)) return LRA_ERR_INVALID;
  if (k < 1 || k > 10 || w < 1 || w > 16 || window < w + k || window > 4096) return lra_set_err(ctx, LRA_ERR_INVALID, "need 1<=k<=10 (20-bit LocalTuple), 1<=w<=16, w+k<=window<=4096");
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  lra_map_state* m = ctx->map;
  if (m->borrowed) return lra_set_err(ctx, LRA_ERR_INVALID, "this context shares another context's reference data: load its own chromosome table first");
  const int n_chrom = (int)m->chrom_pos.size() - 1;
  std::vector<uint64_t> gso; gso.push_back(0);
  std::vector<uint64_t> win_off((size_t)n_chrom + 1, 0);
  for (int c = 0; c < n_chrom; c++) {
    for (uint64_t p_ = m->chrom_pos[c]; p_ < m->chrom_pos[c + 1];) { p_ = std::min<uint64_t>(p_ + (uint64_t)window, m->chrom_pos[c + 1]); gso.push_back(p_); }
    win_off[c + 1] = gso.size() - 1;
  }
  if (gso.size() != n_windows + 1 || memcmp(gso.data(), h_seq_offsets, gso.size() * 8) != 0)
    return lra_set_err(ctx, LRA_ERR_INVALID, "the local index's seqOffsets are not those of the loaded chromosome table at windows of %d bases", window);
  if (h_tuple_bnd[0] != 0 || h_tuple_bnd[n_windows] != n_tuples) return lra_set_err(ctx, LRA_ERR_INVALID, "tupleBoundaries do not cover the tuples");
  for (uint64_t i = 0; i < n_windows; i++) if (h_tuple_bnd[i + 1] < h_tuple_bnd[i]) return lra_set_err(ctx, LRA_ERR_INVALID, "tupleBoundaries decrease");
  m->cell->gen++;
  auto sz = [](size_t n, size_t e) { return (n * e + 255) & ~(size_t)255; };
  const size_t NW = (size_t)n_windows + 2;
  const size_t need = sz((size_t)n_chrom + 1, 8) + sz(NW, 8) + sz((size_t)n_tuples + 1, 4);
  if (m->gli_buf) { (void)hipFree(m->gli_buf); m->gli_buf = nullptr; }
  LRA_HIP_CHECK(ctx, hipMalloc(&m->gli_buf, need + 256));
  char* nb = (char*)m->gli_buf;
  uint64_t* o_win = (uint64_t*)nb; uint64_t* o_bnd = (uint64_t*)(nb + sz((size_t)n_chrom + 1, 8)); uint32_t* o_tup = (uint32_t*)((char*)o_bnd + sz(NW, 8));
  LRA_HIP_CHECK(ctx, hipMemcpy(o_win, win_off.data(), ((size_t)n_chrom + 1) * 8, hipMemcpyHostToDevice));
  LRA_HIP_CHECK(ctx, hipMemcpy(o_bnd, h_tuple_bnd, ((size_t)n_windows + 1) * 8, hipMemcpyHostToDevice));
  if (n_tuples) LRA_HIP_CHECK(ctx, hipMemcpy(o_tup, h_tuples, (size_t)n_tuples * 4, hipMemcpyHostToDevice));
  m->gli = lra_local_index_result{};
  m->gli.n_seqs = n_chrom; m->gli.n_windows = n_windows; m->gli.n_tuples = n_tuples; m->gli.bytes = need;
  m->gli.d_base = nb; m->gli.d_win_off = o_win; m->gli.d_tuple_bnd = o_bnd; m->gli.d_tuples = o_tup;
  m->gli_window = window; m->gli_k = k; m->gli_w = w;
  if (m->d_gso) (void)hipFree(m->d_gso);
  LRA_HIP_CHECK(ctx, hipMalloc((void**)&m->d_gso, gso.size() * 8));
  LRA_HIP_CHECK(ctx, hipMemcpy(m->d_gso, gso.data(), gso.size() * 8, hipMemcpyHostToDevice));
  m->n_gwin = n_windows;
  return LRA_OK;
}

// Several contexts on one GPU (sub-batches on their own HIP streams, so that the serial tails of one sub-batch's kernels overlap the other's work)
// share ONE replica of the reference: dst borrows src's genome, global index + directory, chromosome table and local index.  src must outlive dst.
extern "C" int lra_ctx_share_reference(lra_ctx* dst, lra_ctx* src) {
  if (!dst || !src || dst == src || !src->map || !src->seed || dst->device != src->device) return LRA_ERR_INVALID;
  if (dst->map) return lra_set_err(dst, LRA_ERR_INVALID, "context already holds reference data");
  int rc = lra_seed_share(dst, src);
  if (rc) return rc;
  lra_map_state* m = map_state(dst);
  const lra_map_state* s = src->map;
  m->chrom_pos = s->chrom_pos; m->d_chrom_pos = s->d_chrom_pos; m->gli_buf = s->gli_buf; m->gli = s->gli; m->d_gso = s->d_gso; m->n_gwin = s->n_gwin;
  m->gli_window = s->gli_window; m->gli_k = s->gli_k; m->gli_w = s->gli_w; m->lut = s->lut; m->borrowed = true;
  m->owner_cell = s->borrowed ? s->owner_cell : s->cell; m->owner_generation = s->borrowed ? s->owner_generation : s->cell->gen.load();
  return LRA_OK;
}

// LRA_OK, or LRA_ERR_INVALID when this context borrows reference data (lra_ctx_share_reference) that its owner has replaced since
int lra_map_check_shared(lra_ctx* ctx) {
  int rc = lra_seed_check_shared(ctx);
  if (rc) return rc;
  const lra_map_state* m = ctx->map;
  if (m && m->borrowed && m->owner_cell && (m->owner_cell->dead.load() || m->owner_cell->gen.load() != m->owner_generation))
    return lra_set_err(ctx, LRA_ERR_INVALID, "the context this one shares its reference data with has %s: call lra_ctx_share_reference again",
                       m->owner_cell->dead.load() ? "been destroyed" : "reloaded it");
  return LRA_OK;
}

// the context's reference data, for callers that want to write it to files (lra_write_gli) or hand it to another consumer
extern "C" const char* lra_ctx_genome_ptr(lra_ctx* ctx) { return (ctx && ctx->seed) ? (const char*)ctx->seed->genome : nullptr; }
extern "C" int lra_ctx_local_index(lra_ctx* ctx, lra_local_index_result* out, const uint64_t** d_seq_offsets) {
  if (!ctx || !ctx->map || !ctx->map->gli_buf || !out) return LRA_ERR_INVALID;
  *out = ctx->map->gli;
  if (d_seq_offsets) *d_seq_offsets = ctx->map->d_gso;
  return LRA_OK;
}

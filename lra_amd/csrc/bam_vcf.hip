// lra_amd/csrc/bam_vcf.hip -- lra_bam_vcf: the insertions and deletions of a BAM file's alignments as VCF lines, whole or for a region (gfx950).
// include/lra_hip.h has the interface and the rules; bam_pass.h is the pass it shares with lra_bam_view and lra_bam_depth (the windows, a region's plan,
// the refusals); bam_vcf_walk.h is the walk it shares with lra_bam_svcalls, from the record checks to the compacted variants (its head describes the
// kernels; bam_contained.h is the filter in front of it); bam_vcf_host.h has the arithmetic the host and the kernels share (a variant's lengths, the
// region test, which refusal comes first).
//
// lengths.  For this consumer vc_compact also writes the lengths of a variant's line's four pieces:
//   RNAME \t POS \t . \t | REF | \t ALT | \t 60 \t PASS \t SVTYPE= .. QSTRAND= . \t GT \t 1/1 \n
// One scan places the pieces; its total, in 64 bits, sizes the text.
// emit.  vc_small, a lane per variant: the first and the last piece, the tab in front of ALT, the variant's value record.  vc_bulk, chunk_copy.h's walk:
// the text cut into 4 KiB chunks, a wave each; REF is a copy of genome bytes from chrom_pos[ref] + anchor, ALT the packed SEQ from the anchor's index
// (either nibble parity) through wave_seq (bam_rec.h, the view's).  A 100 kb ALT is 25 waves beside the one that holds a thousand short lines.
#include "common.h"
#include "chunk_copy.h"
#include "scan.h"
#include "bam_pass.h"
#include "bam_keys.h"
#include "bam_vcf_host.h"
#include "bam_vcf_walk.h"
#include <algorithm>
#include <vector>

namespace {

constexpr int CHUNK = 4096;

// a lane per variant: what a lane prints of its line, and its value record
__global__ void __launch_bounds__(256) vc_small(Vc V) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool ins = false, del = false;
  if (j < V.n_var) {
    const Var v = V.var[j];
    ins = !v.del; del = v.del;
    if (V.text) {
      unsigned char* d = V.text + V.poff[4 * j];
      const uint64_t a = V.rname_off[v.ref], b = V.rname_off[v.ref + 1];
      for (uint64_t k = a; k < b; k++) *d++ = (unsigned char)V.rname[k];
      *d++ = '\t'; d = put_u(d, (uint64_t)v.anchor + V.rules.pos_one_based);
      *d++ = '\t'; *d++ = '.'; *d++ = '\t';
      V.text[V.poff[4 * j + 2]] = '\t';
      put_info(V.text + V.poff[4 * j + 3], v.del != 0, v.svlen, V.F.data + v.name_at, v.l_name, v.aq + 1, (v.flag & 16u) != 0);
    }
    if (V.vals) {
      struct lra_bam_vcf_variant x;
      x.record = V.ord_base + v.rec; x.text_off = V.text ? V.poff[4 * j] : 0; x.svlen = v.svlen; x.ref_id = v.ref; x.pos = v.anchor; x.qstart = (uint32_t)(v.aq + 1);
      x.kind = v.del ? 1 : 0; x.strand = (v.flag & 16u) ? 1 : 0; x.pad = 0;
      V.vals[j] = x;
    }
  }
  const unsigned long long bi = __ballot(ins), bd = __ballot(del);
  if ((threadIdx.x & 63) == 0) {
    if (bi) atomicAdd(&V.cnt[N_INS], (unsigned long long)__popcll(bi));
    if (bd) atomicAdd(&V.cnt[N_DEL], (unsigned long long)__popcll(bd));
  }
}

__global__ void __launch_bounds__(256) vc_bulk(Vc V) {
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const int lane = threadIdx.x & 63;
  chunk_walk<CHUNK>(V.n_text, 4 * V.n_var, V.poff, wave, n_waves, [&](uint64_t q, uint64_t b, uint64_t end, uint64_t lo, uint64_t hi) {
    const int part = (int)(q & 3);
    if (part != 1 && part != 2) return;
    const uint64_t wb = b + (part == 2 ? 1 : 0), from = max(lo, wb), to = min(hi, end);
    if (to <= from) return;
    const Var& v = V.var[q >> 2];
    if (part == 1) wave_copy(V.text + from, V.genome + v.g_at + (from - wb), to - from, lane);
    else wave_seq(V.text + from, V.F.data + v.seq_at, v.aq + (from - wb), to - from, lane);
  });
}

}  // namespace

struct lra_bam_vcf : lra_bam_pass {
  lra_bam_vcf_opts O{}; lra_vcf_rules rules{};
  const unsigned char* d_genome = nullptr; const uint64_t* d_chrom_pos = nullptr;
  uint64_t pass_recs = 0;                                      // the records of the pass's windows so far
  // the window
  lra_vcf_walk W; Buf<uint8_t> text; Buf<struct lra_bam_vcf_variant> vals;
  PinBuf<char> h_text; PinBuf<struct lra_bam_vcf_variant> h_vals;
  struct lra_bam_vcf_stats S{};
  uint64_t w_n = 0, w_nv = 0, w_len = 0, w_cnt[N_CNT] = {};    // the window in hand

  lra_bam_vcf() { W.ms_frame_select = &S.ms_frame_select; W.ms_ops = &S.ms_ops; W.ms_walk = &S.ms_walk; W.ms_lengths = &S.ms_lengths; }
  void release_all() { release_pass(); W.release(); text.release(); vals.release(); h_text.release(); h_vals.release(); }
  int take_genome(const char* fn) { return lra_vcf_take_genome(*this, fn, &d_genome, &d_chrom_pos); }
  int begin_pass() { pass_recs = 0; forget(); return W.begin(*this, O.drop_contained != 0); }
  // the pass's consumer
  int window(uint64_t n, uint64_t limit, uint64_t* bad_idx, uint64_t* bad_pos, std::string* bad_why, uint64_t* stop_idx);
  void forget() { w_n = w_nv = w_len = 0; memset(w_cnt, 0, sizeof w_cnt); W.forget(); }
  bool deliver() {
    S.records_read += w_n; S.records_walked += w_cnt[N_WALKED]; S.records_skipped += w_cnt[N_SKIPPED]; S.records_contained += w_cnt[N_CONTAINED];
    S.records_filtered += w_n - w_cnt[N_WALKED] - w_cnt[N_SKIPPED] - w_cnt[N_CONTAINED];
    W.commit(*this);
    S.n_ins += w_cnt[N_INS]; S.n_del += w_cnt[N_DEL]; S.bytes_text += w_len;
    pass_recs += w_n;
    return w_nv != 0;
  }
  int next(struct lra_bam_vcf_piece* piece);
};

int lra_bam_vcf::window(uint64_t n, uint64_t limit, uint64_t* bad_idx, uint64_t* bad_pos, std::string* bad_why, uint64_t* stop_idx) {
  hipStream_t st = ctx->stream;
  *bad_idx = NONE; *stop_idx = NONE;
  forget();
  Vc V; memset(&V, 0, sizeof V);
  V.rules = rules; V.genome = d_genome; V.chrom_pos = d_chrom_pos; V.ord_base = pass_recs;
  if (int rc = W.check(*this, V, n, limit, bad_idx, bad_pos, bad_why)) return rc;
  if (*bad_idx != NONE) return LRA_OK;
  uint64_t nv = 0, total = 0;
  if (int rc = W.walk(*this, V, O.drop_contained != 0, O.want_text != 0, bad_idx, bad_pos, bad_why, stop_idx, &nv, &total, w_cnt)) return rc;
  if (*bad_idx != NONE) return LRA_OK;
  w_n = n;
  if (!nv) return LRA_OK;
  uint64_t dev_text = 0, host_text = 0, value_bytes = 0;
  if (!lra_vcf_piece_bytes(nv, total, (int)O.want_text, (int)O.want_values, &dev_text, &host_text, &value_bytes))
    return fail(LRA_ERR_NOMEM, "lra_bam_vcf: a piece of %llu variants and %llu bytes of text is beyond this machine's addresses", (unsigned long long)nv, (unsigned long long)total);
  {
    Timer T(st);
    if (O.want_text && !grab(text, dev_text)) return fail(LRA_ERR_NOMEM, "lra_bam_vcf: hipMalloc of %llu bytes for a window's text failed", (unsigned long long)total);
    if (O.want_values && !grab(vals, nv)) return fail(LRA_ERR_NOMEM, "lra_bam_vcf: hipMalloc failed for %llu variants", (unsigned long long)nv);
    V.text = O.want_text ? text.p : nullptr; V.n_text = total; V.vals = O.want_values ? vals.p : nullptr;
    hipLaunchKernelGGL(vc_small, dim3(blocks_of(nv)), dim3(256), 0, st, V);
    if (O.want_text) hipLaunchKernelGGL(vc_bulk, dim3(wave_blocks(ctx, (total + CHUNK - 1) / CHUNK)), dim3(256), 0, st, V);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    S.ms_emit += T.stop();
  }
  {
    Timer T(st);
    if (O.want_text) {
      if (!h_text.ensure(host_text, 0, st)) return fail(LRA_ERR_NOMEM, "lra_bam_vcf: hipHostMalloc of %llu bytes for a window's text failed", (unsigned long long)total);
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(h_text.p, text.p, total, hipMemcpyDeviceToHost, st));
    }
    if (O.want_values) {
      if (!h_vals.ensure(nv, 0, st)) return fail(LRA_ERR_NOMEM, "lra_bam_vcf: hipHostMalloc failed for %llu variants", (unsigned long long)nv);
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(h_vals.p, vals.p, value_bytes, hipMemcpyDeviceToHost, st));
    }
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(w_cnt, V.cnt, 8 * N_CNT, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    S.ms_copy += T.stop();
  }
  w_nv = nv; w_len = total;
  return LRA_OK;
}

int lra_bam_vcf::next(struct lra_bam_vcf_piece* piece) {
  memset(piece, 0, sizeof *piece);
  if (!over) if (int rc = take_genome("lra_bam_vcf_next")) { over = true; return rc; }   // (the context may have taken another genome since)
  for (;;) {
    int state = 0;
    if (int rc = step(*this, &state)) return rc;
    if (state == 2) return LRA_OK;
    if (state == 1) {
      piece->n_variants = w_nv; piece->variants = O.want_values ? h_vals.p : nullptr; piece->text = w_len ? h_text.p : nullptr; piece->text_len = w_len;
      return LRA_OK;
    }
  }
}

static_assert(sizeof(struct lra_bam_vcf_variant) == LRA_VCF_VALUE_BYTES, "lra_bam_vcf_variant");

extern "C" int lra_bam_vcf_create(lra_ctx* ctx, const char* bam_path, const char* bai_path, const struct lra_bam_vcf_opts* opts, lra_bam_vcf** out) {
  if (!ctx || !bam_path || !out) return LRA_ERR_INVALID;
  *out = nullptr;
  std::unique_ptr<lra_bam_vcf> d(new lra_bam_vcf());
  if (opts) d->O = *opts; else { d->O.exclude = ~0u; d->O.want_text = 1; }
  d->rules = lra_vcf_rules_of(d->O.require, d->O.exclude, d->O.min_mapq, d->O.min_length, d->O.pos_one_based);
  if (!d->O.want_text && !d->O.want_values) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_bam_vcf_create: neither text nor values are wanted");
  int rc = d->open_files(ctx, "lra_bam_vcf", bam_path, bai_path, d->O.window_bytes);
  if (!rc) rc = d->take_genome("lra_bam_vcf_create");
  if (rc) return pass_create_failed(d.get(), rc);
  // misc behind the pass's words: the window's counts [MISC_CNT, MISC_CNT + N_CNT)
  if (!d->zero_misc()) return pass_create_failed(d.get(), lra_set_err(ctx, LRA_ERR_NOMEM, "lra_bam_vcf_create: hipMalloc failed"));
  *out = d.release();
  return LRA_OK;
}

extern "C" void lra_bam_vcf_destroy(lra_bam_vcf* d) { pass_destroy(d); }

extern "C" int lra_bam_vcf_header(lra_bam_vcf* d, int* n_ref, const char* const** names, const uint64_t** ref_len) {
  return d ? d->header_refs(n_ref, names, ref_len) : LRA_ERR_INVALID;
}

extern "C" int lra_bam_vcf_all(lra_bam_vcf* d) {
  if (!d) return LRA_ERR_INVALID;
  d->over = true;
  if (int rc = d->take_genome("lra_bam_vcf_all")) return rc;
  if (int rc = d->pass_all()) return rc;
  return d->begin_pass();
}

extern "C" int lra_bam_vcf_region(lra_bam_vcf* d, int32_t ref_id, int64_t beg, int64_t end) {
  if (!d) return LRA_ERR_INVALID;
  d->over = true;
  if (int rc = d->take_genome("lra_bam_vcf_region")) return rc;
  if (d->O.drop_contained && beg > 0)
    return lra_set_err(d->ctx, LRA_ERR_INVALID, "lra_bam_vcf_region: drop_contained needs every record of the reference in front of the region (the largest end so far "
                       "decides what is contained): a region with the filter on begins at 0, not at %lld", (long long)beg);
  if (int rc = d->pass_region(ref_id, beg, end)) return rc;
  return d->begin_pass();
}

extern "C" int lra_bam_vcf_next(lra_bam_vcf* d, struct lra_bam_vcf_piece* piece) {
  if (!d || !piece) return LRA_ERR_INVALID;
  LRA_HIP_CHECK(d->ctx, hipSetDevice(d->ctx->device));
  return d->next(piece);
}

extern "C" int lra_bam_vcf_stats(lra_bam_vcf* d, struct lra_bam_vcf_stats* out) {
  if (!d || !out) return LRA_ERR_INVALID;
  *out = d->S;
  d->add_stats(out);
  return LRA_OK;
}

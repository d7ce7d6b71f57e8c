// lra_amd/csrc/bam_svcombine.hip -- lra_sv_combine: two haplotypes' assembly SV calls as the diploid call set -- hom and het lines -- from two sorted BAMs (gfx950).
// The two-haplotype half of the reference's call_assembly_SVs snakefile: the rules Homcalls, Hetcalls and combineHet (bedtools intersect -f F -r with -u and
// -v, the awk that picks the columns, the cat).  include/lra_hip.h has the interface and the rules; bam_svcalls.hip is the one-haplotype pass the object
// owns twice; bam_sv_table.h the rows, the sink and the line emitter shared with it; bam_svcombine_host.h the arithmetic host and kernels share.
//
// passes.  The maternal pass, then the paternal one, each with a sink: a reference's kept rows go, device to device, behind the haplotype's table of the kind
// with their QNAME / ALT bytes, and no text is built.  A table ends up in delivery order: by reference, then NR.
// classify, for each of the four pairings (A, B) = (M_K, P_K), (P_K, M_K), K = INS, DEL.  svc_ref_off, a lane per reference: where B's rows of it begin (a
// binary search on ref), and how many tiles of 256 rows its range takes; one scan places the tiles.  svc_tiles, a block per tile: [lowest START, highest
// END) of its rows.  svc_classify, a lane per row of A: the tiles of its reference's range in B, those that share no base with it passed over, the rows of
// the others tested until one is a partner.  The flag depends on the two tables alone: no atomics.
// emit, for each of the six classes in combineHet's order.  svc_keep: the class's rows of its table (flag == cls); one scan; sv_plen, sv_small, sv_bulk as
// lra_bam_svcalls prints its pieces, the ID's stem the haplotype's, the tail  60 \t INFO \t INFO  or  60 \t PASS \t INFO.
#include "common.h"
#include "chunk_copy.h"
#include "scan.h"
#include "bam_pass.h"
#include "bam_vcf_walk.h"
#include "bam_sv_table.h"
#include "bam_svcalls_host.h"
#include "bam_svcombine_host.h"
#include <stddef.h>
#include <memory>
#include <string>

namespace {

struct SvC {                                                  // one pairing: A's rows against table B
  const SvRow* a; uint64_t na; const SvRow* b; uint64_t nb;
  int32_t n_ref; uint32_t num, den;
  uint64_t* roff; uint32_t* tcnt; const uint64_t* toff;        // per reference: B's first row of it ([n_ref]: nb), its tiles, the first of them
  int64_t* t_lo; int64_t* t_hi;
  uint32_t* flag;                                             // per row of A: 1 with a partner in B
};

__global__ void __launch_bounds__(256) svc_ref_off(SvC C) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r > C.n_ref) return;
  const uint64_t lo = lra_svc_ref_begin(C.b, C.nb, (int32_t)r);
  C.roff[r] = lo;
  if (r < C.n_ref) C.tcnt[r] = (uint32_t)((lra_svc_ref_begin(C.b, C.nb, (int32_t)r + 1) - lo + LRA_SVC_TILE - 1) / LRA_SVC_TILE);
}
// a block per tile (the grid is the bound nb / 256 + n_ref; the blocks behind the last tile leave)
__global__ void __launch_bounds__(LRA_SVC_TILE) svc_tiles(SvC C) {
  __shared__ int64_t lo[LRA_SVC_TILE / 64], hi[LRA_SVC_TILE / 64];
  const uint64_t t = blockIdx.x;
  if (t >= C.toff[C.n_ref]) return;
  int32_t r0 = 0, r1 = C.n_ref;                                // the reference whose tiles hold t: the last r with toff[r] <= t
  while (r1 - r0 > 1) { const int32_t mid = (r0 + r1) >> 1; if (C.toff[mid] <= t) r0 = mid; else r1 = mid; }
  const uint64_t i = C.roff[r0] + (t - C.toff[r0]) * LRA_SVC_TILE + threadIdx.x, end = C.roff[r0 + 1];
  int64_t a = i < end ? C.b[i].start : INT64_MAX, b = i < end ? C.b[i].end : INT64_MIN;
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t a2 = (int64_t)__shfl_xor((unsigned long long)a, o), b2 = (int64_t)__shfl_xor((unsigned long long)b, o);
    a = a2 < a ? a2 : a; b = b2 > b ? b2 : b;
  }
  if ((threadIdx.x & 63) == 0) { lo[threadIdx.x >> 6] = a; hi[threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < LRA_SVC_TILE / 64; w++) { a = lo[w] < a ? lo[w] : a; b = hi[w] > b ? hi[w] : b; }
    C.t_lo[t] = a; C.t_hi[t] = b;
  }
}
__global__ void __launch_bounds__(256) svc_classify(SvC C) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C.na) return;
  const SvRow& r = C.a[i];
  const uint64_t t0 = C.toff[r.ref];
  C.flag[i] = lra_svc_has_partner(r.start, r.end, C.b, C.roff[r.ref], C.roff[r.ref + 1], C.t_lo + t0, C.t_hi + t0, C.num, C.den) ? 1u : 0u;
}
__global__ void __launch_bounds__(256) svc_keep(const uint32_t* flag, uint64_t n, uint32_t cls, uint32_t* kept) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) kept[i] = flag[i] == cls ? 1u : 0u;
}

const char* const HAP_WORD[2] = {"maternal", "paternal"};
// combineHet's cat: hap outside, SVTYPE inside (INS, DEL), the het files in front of the hom files
const struct { int hap, kind, cls; } PIECE[6] = {{0, 0, 0}, {0, 1, 0}, {1, 0, 0}, {1, 1, 0}, {0, 0, 1}, {0, 1, 1}};

}  // namespace

struct lra_sv_combine {
  lra_ctx* ctx = nullptr;
  lra_sv_combine_opts O{}; uint32_t num = 3, den = 10;
  lra_bam_svcalls* pass[2] = {nullptr, nullptr}; lra_sv_sink sink[2];
  int32_t n_ref = 0;
  std::string stem[2][2]; Buf<char> d_stem[2][2];              // [hap][kind]
  bool pending = false; int stage = 6;                         // pending: a run is started and its passes are to be made; stage: the next of PIECE (6: none)
  Buf<uint32_t> flag[2][2], tcnt, kept, kidx, plen; Buf<uint64_t> roff, toff, koff, poff; Buf<int64_t> t_lo, t_hi;
  Buf<uint8_t> text; Buf<struct lra_bam_svcalls_row> vals;
  PinBuf<char> h_text; PinBuf<struct lra_bam_svcalls_row> h_vals;
  struct lra_sv_combine_stats S{};

  template <class T> bool grab(Buf<T>& b, size_t want) { if (b.ensure(want)) return true; (void)hipGetLastError(); return false; }
  int fail(int code, const std::string& why) { (void)hipStreamSynchronize(ctx->stream); pending = false; stage = 6; return lra_set_err(ctx, code, "%s", why.c_str()); }
  void release_all() {
    for (int h = 0; h < 2; h++) {
      if (pass[h]) lra_bam_svcalls_destroy(pass[h]);
      pass[h] = nullptr; sink[h].release();
      for (int k = 0; k < 2; k++) { d_stem[h][k].release(); flag[h][k].release(); }
    }
    tcnt.release(); kept.release(); kidx.release(); plen.release(); roff.release(); toff.release(); koff.release(); poff.release(); t_lo.release(); t_hi.release();
    text.release(); vals.release(); h_text.release(); h_vals.release();
  }
  int run_passes();
  int classify(int ha, int k);
  int emit(int hap, int k, int cls, struct lra_sv_combine_piece* piece);
  int next(struct lra_sv_combine_piece* piece);
};

// both passes to their ends, one after the other: the tables.  A refusal of either refuses the run, the haplotype named.
int lra_sv_combine::run_passes() {
  for (int h = 0; h < 2; h++) sink[h].clear();
  for (int h = 0; h < 2; h++) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      struct lra_bam_svcalls_piece p;
      if (int rc = lra_bam_svcalls_next(pass[h], &p)) {
        const std::string why = ctx->err;
        return fail(rc, std::string("lra_sv_combine: the ") + HAP_WORD[h] + " pass: " + why);
      }
      if (!p.n_rows && !p.text_len) break;
    }
    (h ? S.ms_pass_p : S.ms_pass_m) += wall_ms(t0);
  }
  return LRA_OK;
}

// flag[ha][k]: the rows of haplotype ha's table of kind k that have a partner in the other haplotype's
int lra_sv_combine::classify(int ha, int k) {
  hipStream_t st = ctx->stream;
  const lra_sv_sink& A = sink[ha]; const lra_sv_sink& B = sink[ha ^ 1];
  const uint64_t na = A.n_rows[k], nb = B.n_rows[k];
  if (!na) return LRA_OK;
  if (!grab(flag[ha][k], na)) return fail(LRA_ERR_NOMEM, "lra_sv_combine: hipMalloc failed for " + std::to_string(na) + " rows");
  if (!nb) { LRA_HIP_CHECK(ctx, hipMemsetAsync(flag[ha][k].p, 0, 4 * na, st)); return LRA_OK; }
  const uint64_t tile_cap = nb / LRA_SVC_TILE + (uint64_t)n_ref + 1;
  if (!(grab(roff, (size_t)n_ref + 1) && grab(tcnt, (size_t)n_ref + 1) && grab(toff, (size_t)n_ref + 2) && grab(t_lo, tile_cap) && grab(t_hi, tile_cap)))
    return fail(LRA_ERR_NOMEM, "lra_sv_combine: hipMalloc failed for the tiles of " + std::to_string(nb) + " rows");
  SvC C; memset(&C, 0, sizeof C);
  C.a = A.rows[k].p; C.na = na; C.b = B.rows[k].p; C.nb = nb; C.n_ref = n_ref; C.num = num; C.den = den;
  C.roff = roff.p; C.tcnt = tcnt.p; C.toff = toff.p; C.t_lo = t_lo.p; C.t_hi = t_hi.p; C.flag = flag[ha][k].p;
  hipLaunchKernelGGL(svc_ref_off, dim3(blocks_of((uint64_t)n_ref + 1)), dim3(256), 0, st, C);
  LRA_HIP_CHECK(ctx, hipGetLastError());
  if (lra_exclusive_scan<uint32_t>(ctx, (long)n_ref, tcnt.p, toff.p)) return fail(LRA_ERR_HIP, "lra_sv_combine: a scan failed");
  hipLaunchKernelGGL(svc_tiles, dim3((unsigned)tile_cap), dim3(LRA_SVC_TILE), 0, st, C);
  hipLaunchKernelGGL(svc_classify, dim3(blocks_of(na)), dim3(256), 0, st, C);
  LRA_HIP_CHECK(ctx, hipGetLastError());
  return LRA_OK;
}

// one class's rows, printed into *piece (n_rows == 0: the class is empty)
int lra_sv_combine::emit(int hap, int k, int cls, struct lra_sv_combine_piece* piece) {
  hipStream_t st = ctx->stream;
  const lra_sv_sink& T = sink[hap];
  const uint64_t m = T.n_rows[k];
  if (!m) return LRA_OK;
  uint64_t nk = 0, total = 0, dev_text = 0, host_text = 0, value_bytes = 0;
  SvF F; memset(&F, 0, sizeof F);
  {
    Timer Tm(st);
    if (!(grab(kept, m) && grab(koff, m + 1) && grab(kidx, m))) return fail(LRA_ERR_NOMEM, "lra_sv_combine: hipMalloc failed for " + std::to_string(m) + " rows");
    hipLaunchKernelGGL(svc_keep, dim3(blocks_of(m)), dim3(256), 0, st, (const uint32_t*)flag[hap][k].p, m, (uint32_t)cls, kept.p);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    if (lra_exclusive_scan<uint32_t>(ctx, (long)m, kept.p, koff.p)) return fail(LRA_ERR_HIP, "lra_sv_combine: a scan failed");
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&nk, koff.p + m, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (!nk) { S.ms_emit += Tm.stop(); return LRA_OK; }
    if (O.want_text && !(grab(plen, 4 * nk) && grab(poff, 4 * nk + 1))) return fail(LRA_ERR_NOMEM, "lra_sv_combine: hipMalloc failed for " + std::to_string(nk) + " rows");
    F.rows = T.rows[k].p; F.m = m; F.kept = kept.p; F.koff = koff.p; F.kidx = kidx.p; F.nk = nk; F.plen = O.want_text ? plen.p : nullptr; F.poff = poff.p;
    F.rname = sink[0].rname; F.rname_off = sink[0].rname_off; F.genome = sink[0].genome; F.bytes = T.bytes[k].p;   // (the two files' reference tables are equal)
    F.stem = d_stem[hap][k].p; F.stem_len = (uint32_t)stem[hap][k].size(); F.del = k; F.one_based = O.pos_one_based ? 1u : 0u; F.vcf_columns = 1;
    F.tail = O.filter_pass ? 0u : 1u; F.hap_cls = (uint32_t)hap | ((uint32_t)cls << 8);
    hipLaunchKernelGGL(sv_plen, dim3(blocks_of(m)), dim3(256), 0, st, F);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    if (O.want_text) {
      if (lra_exclusive_scan<uint32_t>(ctx, (long)(4 * nk), plen.p, poff.p)) return fail(LRA_ERR_HIP, "lra_sv_combine: a scan failed");
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(&total, poff.p + 4 * nk, 8, hipMemcpyDeviceToHost, st));
      LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    if (!lra_sv_piece_bytes(nk, total, (int)O.want_text, (int)O.want_values, &dev_text, &host_text, &value_bytes))
      return fail(LRA_ERR_NOMEM, "lra_sv_combine: a piece of " + std::to_string(nk) + " rows and " + std::to_string(total) + " bytes of text is beyond this machine's addresses");
    if (O.want_text && !grab(text, dev_text)) return fail(LRA_ERR_NOMEM, "lra_sv_combine: hipMalloc of " + std::to_string(total) + " bytes for a piece's text failed");
    if (O.want_values && !grab(vals, nk)) return fail(LRA_ERR_NOMEM, "lra_sv_combine: hipMalloc failed for " + std::to_string(nk) + " rows");
    F.text = O.want_text ? text.p : nullptr; F.n_text = total; F.vals = O.want_values ? vals.p : nullptr;
    hipLaunchKernelGGL(sv_small, dim3(blocks_of(nk)), dim3(256), 0, st, F);
    if (O.want_text) hipLaunchKernelGGL(sv_bulk, dim3(wave_blocks(ctx, (total + SV_CHUNK - 1) / SV_CHUNK)), dim3(256), 0, st, F);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    S.ms_emit += Tm.stop();
  }
  {
    Timer Tm(st);
    if (O.want_text) {
      if (!h_text.ensure(host_text, 0, st)) return fail(LRA_ERR_NOMEM, "lra_sv_combine: hipHostMalloc of " + std::to_string(total) + " bytes for a piece's text failed");
      if (total) LRA_HIP_CHECK(ctx, hipMemcpyAsync(h_text.p, text.p, total, hipMemcpyDeviceToHost, st));
    }
    if (O.want_values) {
      if (!h_vals.ensure(nk, 0, st)) return fail(LRA_ERR_NOMEM, "lra_sv_combine: hipHostMalloc failed for " + std::to_string(nk) + " rows");
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(h_vals.p, vals.p, value_bytes, hipMemcpyDeviceToHost, st));
    }
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    S.ms_copy += Tm.stop();
  }
  S.bytes_text += total;
  uint64_t* count[6] = {&S.het_m_ins, &S.het_m_del, &S.het_p_ins, &S.het_p_del, &S.hom_ins, &S.hom_del};
  *count[cls ? 4 + k : 2 * hap + k] += nk;
  piece->n_rows = nk; piece->rows = O.want_values ? (const struct lra_sv_combine_row*)h_vals.p : nullptr; piece->text = total ? h_text.p : nullptr; piece->text_len = total;
  piece->hap = (uint32_t)hap; piece->kind = (uint32_t)k; piece->cls = (uint32_t)cls;
  return LRA_OK;
}

int lra_sv_combine::next(struct lra_sv_combine_piece* piece) {
  hipStream_t st = ctx->stream;
  memset(piece, 0, sizeof *piece);
  if (pending) {
    pending = false;
    if (int rc = run_passes()) return rc;
    Timer Tm(st);
    for (int h = 0; h < 2; h++) for (int k = 0; k < 2; k++) if (int rc = classify(h, k)) return rc;
    for (int k = 0; k < 2; k++) {                              // the paternal rows with a partner, which are printed nowhere: counted here
      const uint64_t n = sink[1].n_rows[k];
      uint64_t with = 0;
      if (!n) continue;
      if (!grab(koff, n + 1)) return fail(LRA_ERR_NOMEM, "lra_sv_combine: hipMalloc failed for " + std::to_string(n) + " rows");
      if (lra_exclusive_scan<uint32_t>(ctx, (long)n, flag[1][k].p, koff.p)) return fail(LRA_ERR_HIP, "lra_sv_combine: a scan failed");
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(&with, koff.p + n, 8, hipMemcpyDeviceToHost, st));
      LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
      (k ? S.partnered_p_del : S.partnered_p_ins) += with;
    }
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    S.ms_classify += Tm.stop();
    S.runs++;
    stage = 0;
  }
  while (stage < 6) {
    const int s = stage++;
    if (int rc = emit(PIECE[s].hap, PIECE[s].kind, PIECE[s].cls, piece)) return rc;
    if (piece->n_rows) return LRA_OK;
  }
  return LRA_OK;                                               // the end piece
}

static_assert(sizeof(struct lra_sv_combine_row) == sizeof(struct lra_bam_svcalls_row) && offsetof(struct lra_sv_combine_row, hap) == offsetof(struct lra_bam_svcalls_row, pad) &&
              offsetof(struct lra_sv_combine_row, cls) == offsetof(struct lra_bam_svcalls_row, pad) + 1 && offsetof(struct lra_sv_combine_row, kind) == offsetof(struct lra_bam_svcalls_row, kind),
              "lra_sv_combine_row is lra_bam_svcalls_row with hap and cls in its pad");

extern "C" int lra_sv_combine_create(lra_ctx* ctx, const char* bam_m, const char* bai_m, const char* bam_p, const char* bai_p, const struct lra_sv_combine_opts* opts,
                                     lra_sv_combine** out) {
  if (!ctx || !bam_m || !bam_p || !out) return LRA_ERR_INVALID;
  *out = nullptr;
  std::unique_ptr<lra_sv_combine> d(new lra_sv_combine());
  d->ctx = ctx;
  if (opts) d->O = *opts; else { d->O.exclude = ~0u; d->O.want_text = 1; d->O.drop_contained = 1; d->O.min_size = 40; }
  if (!lra_svc_frac(d->O.frac_num, d->O.frac_den, &d->num, &d->den))
    return lra_set_err(ctx, LRA_ERR_INVALID, "lra_sv_combine_create: the fraction %u / %u is not in (0, 1]", d->O.frac_num, d->O.frac_den);
  if (!d->O.want_text && !d->O.want_values) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_sv_combine_create: neither text nor values are wanted");
  if (!lra_sv_name_ok(d->O.aligner)) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_sv_combine_create: aligner is a printable word without blanks");
  const char* bam[2] = {bam_m, bam_p}; const char* bai[2] = {bai_m, bai_p};
  int rc = LRA_OK;
  for (int h = 0; h < 2 && !rc; h++) {
    struct lra_bam_svcalls_opts P; memset(&P, 0, sizeof P);
    P.require = d->O.require; P.exclude = d->O.exclude; P.min_mapq = d->O.min_mapq; P.min_size = d->O.min_size; P.drop_contained = d->O.drop_contained;
    P.want_values = 1; P.window_bytes = d->O.window_bytes; P.aligner = d->O.aligner; P.hap = HAP_WORD[h];
    rc = lra_bam_svcalls_create(ctx, bam[h], bai[h], &P, &d->pass[h]);
    if (rc) break;
    lra_bam_svcalls_set_sink(d->pass[h], &d->sink[h]);
    for (int k = 0; k < 2; k++) d->stem[h][k] = lra_sv_id_stem(d->O.aligner, HAP_WORD[h], k);
  }
  d->O.aligner = nullptr;                                      // (the caller's string is not kept)
  if (!rc) {
    // the two reference tables: each equals the context's (the passes' create), and they equal each other name by name
    int n[2] = {0, 0}; const char* const* nm[2] = {nullptr, nullptr}; const uint64_t* len[2] = {nullptr, nullptr};
    for (int h = 0; h < 2; h++) (void)lra_bam_svcalls_header(d->pass[h], &n[h], &nm[h], &len[h]);
    if (n[0] != n[1]) rc = lra_set_err(ctx, LRA_ERR_INVALID, "lra_sv_combine_create: %s has %d references, %s has %d", bam_p, n[1], bam_m, n[0]);
    for (int i = 0; !rc && i < n[0]; i++) {
      if (strcmp(nm[0][i], nm[1][i]) != 0)
        rc = lra_set_err(ctx, LRA_ERR_INVALID, "lra_sv_combine_create: %s: reference %d is named %s, in %s it is %s", bam_p, i, nm[1][i], bam_m, nm[0][i]);
      else if (len[0][i] != len[1][i])
        rc = lra_set_err(ctx, LRA_ERR_INVALID, "lra_sv_combine_create: %s: reference %d (%s) has length %llu, in %s it has %llu", bam_p, i, nm[1][i],
                         (unsigned long long)len[1][i], bam_m, (unsigned long long)len[0][i]);
    }
    d->n_ref = n[0];
  }
  bool ok = !rc;
  for (int h = 0; ok && h < 2; h++)
    for (int k = 0; ok && k < 2; k++)
      ok = d->d_stem[h][k].ensure(d->stem[h][k].size() + 1) && hipMemcpyAsync(d->d_stem[h][k].p, d->stem[h][k].data(), d->stem[h][k].size(), hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
  ok = ok && hipStreamSynchronize(ctx->stream) == hipSuccess;
  if (!ok) {
    if (!rc) { (void)hipGetLastError(); rc = lra_set_err(ctx, LRA_ERR_NOMEM, "lra_sv_combine_create: hipMalloc failed"); }
    d->release_all();
    return rc;
  }
  *out = d.release();
  return LRA_OK;
}

extern "C" void lra_sv_combine_destroy(lra_sv_combine* d) {
  if (!d) return;
  (void)hipSetDevice(d->ctx->device);
  (void)hipStreamSynchronize(d->ctx->stream);
  d->release_all();
  delete d;
}

extern "C" int lra_sv_combine_header(lra_sv_combine* d, int* n_ref, const char* const** names, const uint64_t** ref_len) {
  return d ? lra_bam_svcalls_header(d->pass[0], n_ref, names, ref_len) : LRA_ERR_INVALID;
}

extern "C" int lra_sv_combine_set_mask(lra_sv_combine* d, uint64_t n, const int32_t* ref_id, const int64_t* beg, const int64_t* end) {
  if (!d) return LRA_ERR_INVALID;
  d->pending = false; d->stage = 6;                            // (a run in hand ends: its rows were tested against the mask before)
  for (int h = 0; h < 2; h++) if (int rc = lra_bam_svcalls_set_mask(d->pass[h], n, ref_id, beg, end)) return rc;
  return LRA_OK;
}

extern "C" int lra_sv_combine_all(lra_sv_combine* d) {
  if (!d) return LRA_ERR_INVALID;
  d->pending = false; d->stage = 6;
  for (int h = 0; h < 2; h++) if (int rc = lra_bam_svcalls_all(d->pass[h])) return rc;
  d->pending = true;
  return LRA_OK;
}

extern "C" int lra_sv_combine_region(lra_sv_combine* d, int32_t ref_id, int64_t beg, int64_t end) {
  if (!d) return LRA_ERR_INVALID;
  d->pending = false; d->stage = 6;
  for (int h = 0; h < 2; h++) if (int rc = lra_bam_svcalls_region(d->pass[h], ref_id, beg, end)) return rc;
  d->pending = true;
  return LRA_OK;
}

extern "C" int lra_sv_combine_next(lra_sv_combine* d, struct lra_sv_combine_piece* piece) {
  if (!d || !piece) return LRA_ERR_INVALID;
  LRA_HIP_CHECK(d->ctx, hipSetDevice(d->ctx->device));
  return d->next(piece);
}

extern "C" int lra_sv_combine_stats(lra_sv_combine* d, struct lra_sv_combine_stats* out) {
  if (!d || !out) return LRA_ERR_INVALID;
  *out = d->S;
  for (int h = 0; h < 2; h++) if (int rc = lra_bam_svcalls_stats(d->pass[h], &out->pass[h])) return rc;
  return LRA_OK;
}

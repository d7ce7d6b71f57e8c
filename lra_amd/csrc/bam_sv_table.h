// lra_amd/csrc/bam_sv_table.h -- what lra_bam_svcalls (bam_svcalls.hip) and lra_sv_combine (bam_svcombine.hip) share: a row of a kind's table, the array
// the tables grow in, the line emitter -- sv_plen, sv_small, sv_bulk over the rows a flag array keeps -- and the sink through which a pass hands its kept rows
// to the object that combines two haplotypes.  The sink is internal: no part of the ABI.
#pragma once
#include "common.h"
#include "chunk_copy.h"
#include "bam_pass.h"
#include "bam_vcf_walk.h"

// (the three types below have external linkage: lra_bam_svcalls_set_sink crosses translation units)
struct SvRow {                                                 // a row of a kind's table
  int64_t start, end, svlen; uint64_t nr, record, g_at, ref_len, alt_len, b_off;   // b_off: QNAME then ALT in the kind's bytes
  int32_t ref; uint32_t qstart, l_name, reverse;
};

// an array whose first items survive its growth
template <typename T> struct KeepBuf {
  T* p = nullptr; size_t n = 0;
  bool ensure(size_t want, size_t keep, hipStream_t st) {
    if (want <= n) return true;
    const size_t m = want + want / 2 + 64;
    T* q = nullptr;
    if (hipMalloc((void**)&q, m * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (keep && (hipMemcpyAsync(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) { (void)hipFree(q); return false; }
    if (p) { (void)hipStreamSynchronize(st); (void)hipFree(p); }
    p = q; n = m;
    return true;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

// One haplotype's kept rows, [0] INS and [1] DEL, by reference and then NR, with their QNAME / ALT bytes: what a pass with a sink appends, a reference at a
// time, instead of printing.  The pointers are the pass's own arrays and the context's genome, for the lines printed from the tables later.
struct lra_sv_sink {
  KeepBuf<SvRow> rows[2]; KeepBuf<uint8_t> bytes[2]; uint64_t n_rows[2] = {0, 0}, n_bytes[2] = {0, 0};
  const char* rname = nullptr; const uint64_t* rname_off = nullptr; const unsigned char* genome = nullptr;
  void clear() { for (int k = 0; k < 2; k++) n_rows[k] = n_bytes[k] = 0; }
  void release() { for (int k = 0; k < 2; k++) { rows[k].release(); bytes[k].release(); } clear(); }
};

namespace {

constexpr int SV_CHUNK = 4096;

// ---- the lines of the rows a flag array keeps ----------------------------------------------------------------------------------------------------------------------
// tail 0:  \t 60 \t PASS \t INFO \t GT \t 1/1 \n     tail 1:  \t 60 \t INFO \t INFO \t GT \t 1/1 \n  (the combine's awk prints $9 in the FILTER column too)
struct SvF {
  const SvRow* rows; uint64_t m;                              // the table's head: rows [0, m), NR order (lra_bam_svcalls: one reference)
  unsigned long long* misc;
  int64_t* t_lo; int64_t* t_hi;                               // per SV_TILE rows in NR order: the lowest START and the highest END
  uint32_t* deg; uint64_t* eoff; uint32_t* in;
  uint32_t* st_a; uint32_t* st_b;
  uint32_t* kept; uint64_t* koff; uint32_t* kidx; uint64_t nk;
  uint32_t* plen; uint64_t* poff;
  const char* rname; const uint64_t* rname_off; const unsigned char* genome; const uint8_t* bytes;
  const char* stem; uint32_t stem_len; int del; uint32_t one_based, vcf_columns, tail, hap_cls;   // hap_cls: the values' hap | cls << 8 (lra_bam_svcalls: 0, its pad)
  unsigned char* text; uint64_t n_text; struct lra_bam_svcalls_row* vals;
};

__device__ __forceinline__ uint32_t sv_head_len(const SvF& F, const SvRow& r) {
  const uint32_t name = (uint32_t)(F.rname_off[r.ref + 1] - F.rname_off[r.ref]);
  return name + 1u + (uint32_t)ndig((uint64_t)r.start + F.one_based) + 1u + (F.vcf_columns ? 0u : (uint32_t)ndig((uint64_t)r.end + F.one_based) + 1u) + F.stem_len + (uint32_t)ndig(r.nr) + 1u;
}
__global__ void __launch_bounds__(256) sv_plen(SvF F) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= F.m || !F.kept[i]) return;
  const uint64_t j = F.koff[i];
  F.kidx[j] = (uint32_t)i;
  if (!F.plen) return;
  const SvRow& r = F.rows[i];
  F.plen[4 * j] = sv_head_len(F, r); F.plen[4 * j + 1] = (uint32_t)r.ref_len; F.plen[4 * j + 2] = 1u + (uint32_t)r.alt_len;   // (32 bits: bam_vcf_walk.h's vc_compact says why)
  F.plen[4 * j + 3] = info_len(r.svlen, r.l_name, r.qstart) + (F.tail ? info_body_len(r.svlen, r.l_name, r.qstart) + 1u - LIT_LEN(T_PASS) : 0u);
}
__global__ void __launch_bounds__(256) sv_small(SvF F) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= F.nk) return;
  const SvRow& r = F.rows[F.kidx[j]];
  if (F.text) {
    unsigned char* d = F.text + F.poff[4 * j];
    const uint64_t a = F.rname_off[r.ref], b = F.rname_off[r.ref + 1];
    for (uint64_t k = a; k < b; k++) *d++ = (unsigned char)F.rname[k];
    *d++ = '\t'; d = put_u(d, (uint64_t)r.start + F.one_based);
    if (!F.vcf_columns) { *d++ = '\t'; d = put_u(d, (uint64_t)r.end + F.one_based); }
    *d++ = '\t';
    for (uint32_t k = 0; k < F.stem_len; k++) *d++ = (unsigned char)F.stem[k];
    d = put_u(d, r.nr); *d++ = '\t';
    F.text[F.poff[4 * j + 2]] = '\t';
    unsigned char* t = F.text + F.poff[4 * j + 3];
    if (!F.tail) put_info(t, F.del != 0, r.svlen, F.bytes + r.b_off, r.l_name, r.qstart, r.reverse != 0);
    else {
      t = put_lit(t, T_QUAL);
      for (int twice = 0; twice < 2; twice++) {
        t = put_info_body(t, F.del != 0, r.svlen, F.bytes + r.b_off, r.l_name, r.qstart, r.reverse != 0);
        if (!twice) *t++ = '\t';
      }
      put_lit(t, T_END);
    }
  }
  if (F.vals) {
    struct lra_bam_svcalls_row x;
    x.record = r.record; x.text_off = F.text ? F.poff[4 * j] : 0; x.nr = r.nr; x.start = r.start; x.end = r.end; x.svlen = r.svlen; x.ref_id = r.ref; x.qstart = r.qstart;
    x.kind = F.del ? 1 : 0; x.strand = (uint8_t)r.reverse; x.pad = (uint16_t)F.hap_cls; x.pad2 = 0;
    F.vals[j] = x;
  }
}
__global__ void __launch_bounds__(256) sv_bulk(SvF F) {
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const int lane = threadIdx.x & 63;
  chunk_walk<SV_CHUNK>(F.n_text, 4 * F.nk, F.poff, wave, n_waves, [&](uint64_t q, uint64_t b, uint64_t end, uint64_t lo, uint64_t hi) {
    const int part = (int)(q & 3);
    if (part != 1 && part != 2) return;
    const uint64_t wb = b + (part == 2 ? 1 : 0), from = max(lo, wb), to = min(hi, end);
    if (to <= from) return;
    const SvRow& r = F.rows[F.kidx[q >> 2]];
    const unsigned char* src = part == 1 ? F.genome + r.g_at : F.bytes + r.b_off + r.l_name;
    wave_copy(F.text + from, src + (from - wb), to - from, lane);
  });
}

}  // namespace

// the pass appends every reference's kept rows to *sink (owned by the caller, alive as long as the pass) and prints nothing; nullptr: as created
struct lra_bam_svcalls;
__attribute__((visibility("hidden"))) void lra_bam_svcalls_set_sink(lra_bam_svcalls* d, lra_sv_sink* sink);

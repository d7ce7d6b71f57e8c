// lra_amd/csrc/svsig_text.hip -- the text of a batch's SV signatures (MapRead's svsigstrm: the lines Alignment::Printsvsig writes, Alignment.h:374-399) on
// the device (gfx950), from the records lra_sv_signatures_batch (svsig.hip) leaves.  One line per signature,
//     chrom \t readName \t t_start \t end \t len \t INS|DEL \t bases \n
// byte for byte what lra_map_svsig_host (map_output.hip) appends field by field on the host.
//
// Shape, as the other text builders (records.hip, md.hip, pairwise.hip): svt_count, a lane per signature, finds its alignment by binary search in sig_off
// (as sv_emit does) and writes the line's bytes -- the two names, three decimal widths, the bases and 10 fixed bytes (6 tabs, INS / DEL, the newline); 0 for
// a skipped alignment.  A scan (scan.h) gives every line its place.  svt_head, a lane per signature, writes everything up to the last tab and the newline,
// and lane a reads aln_off[a] off the scan.  The bases go through chunk_copy.h's loop: the OUTPUT cut into chunks of SVT_CHUNK bytes, one wave each, aligned
// dwords -- a line is one string of the loop of which only a WINDOW (the bases) is copied, the rest being svt_head's; a 50 kb deletion is a dozen waves and
// a chunk of 1-base insertions is one.  The host reads one number: the text's bytes.
#include "common.h"
#include "chunk_copy.h"
#include "scan.h"
#include <algorithm>

namespace {

constexpr int SVT_CHUNK = 4096;                              // output bytes per wave of svt_copy
constexpr int SVT_FIXED = 10;                                // 6 tabs, "INS" / "DEL", '\n'

__device__ __forceinline__ int dec_width(uint32_t v) {
  return v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5 : v < 1000000u ? 6 : v < 10000000u ? 7 : v < 100000000u ? 8 : v < 1000000000u ? 9 : 10;
}
__device__ __forceinline__ unsigned char* put_dec(unsigned char* w, uint32_t v) {   // -> behind the digits
  const int width = dec_width(v);
  for (int k = width - 1; k >= 0; k--) { w[k] = (unsigned char)('0' + v % 10u); v /= 10u; }
  return w + width;
}

struct SvtArgs {
  int n_aln, n_reads, n_chrom; uint64_t n_sig;
  const uint64_t* sig_off; const lra_svsig_rec* rec; const unsigned char* seq;
  const uint32_t* aln_read; const int32_t* chrom; const uint8_t* skip;           // per alignment (skip NULL: none)
  const unsigned char* rname; const uint64_t* rname_off; const unsigned char* cname; const uint64_t* cname_off;
  uint32_t* w; uint32_t* aln;                                  // per signature: its line's bytes, its alignment
  const uint64_t* at;                                          // the bytes' exclusive prefix [n_sig + 1]
  uint64_t* aln_off; unsigned char* text; uint64_t n_text;     // the result
};

__device__ __forceinline__ uint32_t sv_end(const lra_svsig_rec& r) { return r.kind == LRA_SV_DEL ? (uint32_t)(r.t_start + r.len - 1) : r.t_start; }
// a name of a table: its bytes and length (an index outside the table names nothing)
__device__ __forceinline__ const unsigned char* name_of(const unsigned char* blob, const uint64_t* off, int64_t i, int n, uint64_t& len) {
  len = 0;
  if (i < 0 || i >= n) return blob;
  len = off[i + 1] - off[i];
  return blob + off[i];
}

__global__ void __launch_bounds__(256) svt_count(SvtArgs A) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= A.n_sig) return;
  int lo = 0, hi = A.n_aln - 1;                                // the alignment of signature s: the first whose signatures end behind it
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (A.sig_off[mid + 1] <= s) lo = mid + 1; else hi = mid; }
  A.aln[s] = (uint32_t)lo;
  uint64_t n = 0;
  if (!(A.skip && A.skip[lo])) {
    const lra_svsig_rec r = A.rec[s];
    uint64_t nc, nr;
    name_of(A.cname, A.cname_off, A.chrom[lo], A.n_chrom, nc);
    name_of(A.rname, A.rname_off, A.aln_read[lo], A.n_reads, nr);
    n = nc + nr + dec_width(r.t_start) + dec_width(sv_end(r)) + dec_width(r.len) + r.len + SVT_FIXED;
  }
  A.w[s] = (uint32_t)n;
}

// lane i: the head and the newline of line i, and aln_off[i] of alignment i (i = n_aln: the total)
__global__ void __launch_bounds__(256) svt_head(SvtArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= (uint64_t)A.n_aln) A.aln_off[i] = A.at[A.sig_off[i]];
  if (i >= A.n_sig) return;
  const uint64_t at = A.at[i], end = A.at[i + 1];
  if (end == at || end > A.n_text) return;                     // a skipped alignment's; (nothing is written past the result, whatever the counts say)
  const uint32_t a = A.aln[i];
  const lra_svsig_rec r = A.rec[i];
  uint64_t nc, nr;
  const unsigned char* c = name_of(A.cname, A.cname_off, A.chrom[a], A.n_chrom, nc);
  const unsigned char* q = name_of(A.rname, A.rname_off, A.aln_read[a], A.n_reads, nr);
  unsigned char* w = A.text + at;
  for (uint64_t k = 0; k < nc; k++) w[k] = c[k];
  w += nc; *w++ = '\t';
  for (uint64_t k = 0; k < nr; k++) w[k] = q[k];
  w += nr; *w++ = '\t';
  w = put_dec(w, r.t_start); *w++ = '\t';
  w = put_dec(w, sv_end(r)); *w++ = '\t';
  w = put_dec(w, r.len); *w++ = '\t';
  const bool del = r.kind == LRA_SV_DEL;
  w[0] = del ? 'D' : 'I'; w[1] = del ? 'E' : 'N'; w[2] = del ? 'L' : 'S'; w[3] = '\t';
  A.text[end - 1] = '\n';
}

// one wave per chunk of the output bytes (chunk_copy.h): of line p the bases alone, which end in front of its newline
__global__ void __launch_bounds__(256) svt_copy(SvtArgs A) {
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  chunk_copy<SVT_CHUNK>(A.text, A.n_text, A.n_sig, A.at, [&](uint64_t p) { return A.seq + A.rec[p].seq_off; }, wave, n_waves, threadIdx.x & 63,
                        [&](uint64_t p, uint64_t& b, uint64_t& e) {
                          const uint64_t n = A.rec[p].len;
                          if (e - b < n + SVT_FIXED) { e = b; return; }
                          e -= 1; b = e - n;
                        });
}

inline size_t sz(size_t n, size_t e) { return (n * e + 255) & ~(size_t)255; }
}  // namespace

extern "C" int lra_svsig_text_batch(lra_ctx* ctx, const lra_svsig_result* sv, const uint32_t* d_aln_read, const int32_t* d_chrom, const uint8_t* d_skip,
                                    int n_reads, const char* d_read_names, const uint64_t* d_read_name_off, int n_chrom, const char* d_chrom_names,
                                    const uint64_t* d_chrom_name_off, lra_svsig_text_result* out) {
  if (!ctx || !sv || !out || sv->n_aln < 0 || n_reads < 0 || n_chrom < 0) return LRA_ERR_INVALID;
  const uint64_t nS = sv->n_sig;
  const size_t nA = (size_t)sv->n_aln;
  if (nS && (!nA || !sv->d_sig_off || !sv->d_sig || (sv->n_seq_bytes && !sv->d_seq) || !d_aln_read || !d_chrom || !d_read_names || !d_read_name_off ||
             !d_chrom_names || !d_chrom_name_off))
    return LRA_ERR_INVALID;
  memset(out, 0, sizeof(*out));
  out->n_aln = sv->n_aln; out->n_sig = nS;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (!nS) {                                                   // no line: aln_off is zeros, nothing is launched
    uint64_t* off = (uint64_t*)lra_ensure(ctx, 83, sz(nA + 1, 8));
    if (!off) return LRA_ERR_NOMEM;
    LRA_HIP_CHECK(ctx, hipMemsetAsync(off, 0, (nA + 1) * 8, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    out->d_aln_off = off;
    return LRA_OK;
  }
  SvtArgs A; memset(&A, 0, sizeof A);
  A.n_aln = sv->n_aln; A.n_reads = n_reads; A.n_chrom = n_chrom; A.n_sig = nS;
  A.sig_off = sv->d_sig_off; A.rec = sv->d_sig; A.seq = (const unsigned char*)sv->d_seq;
  A.aln_read = d_aln_read; A.chrom = d_chrom; A.skip = d_skip;
  A.rname = (const unsigned char*)d_read_names; A.rname_off = d_read_name_off; A.cname = (const unsigned char*)d_chrom_names; A.cname_off = d_chrom_name_off;
  // scratch 0 (dead at return): per signature -- its line's bytes, its alignment, the bytes' prefix
  char* w = (char*)lra_scratch(ctx, 0, 2 * sz(nS, 4) + sz(nS + 1, 8));
  if (!w) return LRA_ERR_NOMEM;
  A.w = (uint32_t*)w; w += sz(nS, 4);
  A.aln = (uint32_t*)w; w += sz(nS, 4);
  uint64_t* at = (uint64_t*)w;
  A.at = at;
  uint64_t total = 0;
  lra_time_begin(ctx, "svsig_text");
  hipLaunchKernelGGL(svt_count, dim3((unsigned)((nS + 255) / 256)), dim3(256), 0, st, A);
  if (lra_exclusive_scan<uint32_t>(ctx, (long)nS, A.w, at)) return LRA_ERR_HIP;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&total, at + nS, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  // 83: the result -- aln_off, the text (+ 64 bytes, as the other texts have)
  char* r = (char*)lra_ensure(ctx, 83, sz(nA + 1, 8) + sz(total + 64, 1));
  if (!r) return LRA_ERR_NOMEM;
  A.aln_off = (uint64_t*)r; A.text = (unsigned char*)(r + sz(nA + 1, 8)); A.n_text = total;
  const uint64_t lanes = std::max<uint64_t>(nS, nA + 1);
  hipLaunchKernelGGL(svt_head, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, A);
  if (total && sv->n_seq_bytes) {
    const uint64_t n_chunks = (total + SVT_CHUNK - 1) / SVT_CHUNK;
    hipLaunchKernelGGL(svt_copy, dim3((unsigned)std::min<uint64_t>((n_chunks + 3) / 4, (uint64_t)ctx->num_cu * 32)), dim3(256), 0, st, A);
  }
  lra_time_end(ctx);
  LRA_HIP_CHECK(ctx, hipGetLastError());
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  out->n_bytes = total; out->d_aln_off = A.aln_off; out->d_text = (const char*)A.text;
  return LRA_OK;
}

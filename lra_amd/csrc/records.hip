// lra_amd/csrc/records.hip -- the record text of a batch (print formats 's', 'P' and 'a') built on the device (gfx950): the CIGAR strings from the runs, and
// the records from a PIECE TABLE the host writes (mapread.hip: lra_map_records_device).
//
// CIGAR text (lra_cigar_text_batch).  Flat over the batch's runs, so an alignment of 10^5 runs is 10^5 lanes like everything else: cg_count writes the
// bytes of every run (its decimal width + the op) and, per alignment, the bytes of its two clips; two scans (scan.h) give every run and every alignment
// its offset -- run x of alignment a lands at T[x] + C[a] + the width of a's leading clip, alignment a's text starts at T[run_off[a]] + C[a] -- and
// cg_emit writes the digits, one lane per run, and the clips, one lane per alignment.  Without clips (the record stage: the clips are short host text)
// C is 0 and no lane looks for its alignment.
//
// Records (lra_records_assemble).  A piece is 16 bytes: a literal (a range of the host's literal blob), a range of a read on one strand, a range of a
// read's qualities, the CIGAR text, the MD:Z value or the pairwise rows (pairwise.hip) of an alignment.  rc_resolve gives every piece its length and source address, a scan its place, and
// rc_copy cuts the OUTPUT into chunks of RC_CHUNK bytes, one wave each, as sv_copy does: the wave finds the first piece under its chunk and copies the
// pieces' parts that lie in it, so a 1 Mb contig's SEQ is 256 waves and a chunk of 200-byte records is one wave.  The destination is written in aligned
// dwords (a lane's dword is put together from the two aligned source dwords around it), bytes at a part's ragged ends.  The loop is chunk_copy.h's, which
// lra_pack_strings_batch (pack_strings.hip) runs too.  rc_rec_off reads every read's
// first byte off the scan.  The host reads one number (the text's bytes), then the text and rec_off in one copy each.
// BAM records (lra_map_records_device_bam) are assembled the same way: three more piece kinds point into the staging arrays bam_encode.hip wrote (an
// alignment's ops, a range's packed bases, a request's phred bytes), and behind the copy rc_block_size writes every record's block_size, which the host
// cannot know (MD and SA:Z are the device's), from the host's list of first pieces and the scan.
#include "common.h"
#include "chunk_copy.h"
#include "records.h"
#include "scan.h"
#include <algorithm>
#include <chrono>

namespace {

constexpr int RC_CHUNK = 4096;                               // output bytes per wave of rc_copy

__device__ __forceinline__ int dec_width(uint32_t v) {
  return v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5 : v < 1000000u ? 6 : v < 10000000u ? 7 : v < 100000000u ? 8 : v < 1000000000u ? 9 : 10;
}
__device__ __forceinline__ void put_dec(unsigned char* w, uint32_t v, int width) {
  for (int k = width - 1; k >= 0; k--) { w[k] = (unsigned char)('0' + v % 10u); v /= 10u; }
}

struct CgArgs {
  int n_aln; uint64_t n_runs;
  const uint32_t* runs; const uint64_t* run_off;
  const int32_t* pre; const int32_t* suf; const uint8_t* clip_op;   // NULL: no clips / 'S'
  uint8_t* w; uint8_t* cw;                                     // bytes per run; per alignment: both clips' bytes
  const uint64_t* T; const uint64_t* C;                        // their exclusive prefixes [n_runs + 1], [n_aln + 1] (C NULL without clips)
  uint64_t* off; unsigned char* text; uint64_t n_text;        // the result
};

__device__ __forceinline__ int clip_width(int32_t c) { return c > 0 ? dec_width((uint32_t)c) + 1 : 0; }

__global__ void __launch_bounds__(256) cg_count(CgArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < A.n_runs) A.w[i] = (uint8_t)(dec_width(A.runs[i] >> 4) + 1);
  if (A.cw && i < (uint64_t)A.n_aln) A.cw[i] = (uint8_t)(clip_width(A.pre ? A.pre[i] : 0) + clip_width(A.suf ? A.suf[i] : 0));
}

// lane i: the text of run i, and off[i] + the clips of alignment i (i = n_aln: the total)
__global__ void __launch_bounds__(256) cg_emit(CgArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= (uint64_t)A.n_aln) {
    const uint64_t at = A.T[A.run_off[i]] + (A.C ? A.C[i] : 0);
    A.off[i] = at;
    if (A.C && i < (uint64_t)A.n_aln) {
      const char op = A.clip_op ? (char)A.clip_op[i] : 'S';
      const int32_t p = A.pre ? A.pre[i] : 0, s = A.suf ? A.suf[i] : 0;
      const int pw = clip_width(p), sw = clip_width(s);
      const uint64_t end = A.T[A.run_off[i + 1]] + A.C[i + 1];             // = at + pw + the runs' text + sw
      if (pw && at + pw <= A.n_text) { put_dec(A.text + at, (uint32_t)p, pw - 1); A.text[at + pw - 1] = (unsigned char)op; }
      if (sw && end <= A.n_text && end >= (uint64_t)sw) { put_dec(A.text + end - sw, (uint32_t)s, sw - 1); A.text[end - 1] = (unsigned char)op; }
    }
  }
  if (i >= A.n_runs) return;
  uint64_t at = A.T[i];
  if (A.C) {
    int lo = 0, hi = A.n_aln - 1;                              // the alignment of run i: the first whose runs end behind it
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (A.run_off[mid + 1] <= i) lo = mid + 1; else hi = mid; }
    at += A.C[lo] + clip_width(A.pre ? A.pre[lo] : 0);
  }
  const uint32_t r = A.runs[i];
  const int wd = dec_width(r >> 4);
  if (at + wd + 1 > A.n_text) return;                          // (nothing is written past the result, whatever the counts say)
  put_dec(A.text + at, r >> 4, wd);
  A.text[at + wd] = (unsigned char)("=XID????????????"[r & 15]);
}

// ---- the records ----------------------------------------------------------------------------------------------------------------------------------
struct RcArgs {
  uint64_t n_pieces; int n_reads; uint64_t n_aln;
  const lra_rec_piece* piece; const uint64_t* read_piece;      // [n_pieces], [n_reads + 1]: a read's first piece
  const unsigned char* blob; uint64_t blob_bytes;
  const unsigned char* strands; const uint64_t* read_off; uint64_t rc_base;
  const unsigned char* qual; const uint64_t* qual_off;         // NULL: no read has qualities
  const unsigned char* cg; const uint64_t* cg_off;
  const unsigned char* md; const uint64_t* md_off;             // NULL: no MD pieces
  const unsigned char* pw; const uint64_t* pw_off;             // NULL: no PAIRWISE pieces
  const uint32_t* bcg; const uint64_t* bcg_off;                // NULL: no BAM_CIGAR pieces
  const unsigned char* pseq; const uint64_t* pseq_off; uint64_t n_pseq;      // NULL: no BAM_SEQ pieces
  const unsigned char* phred; const uint64_t* phred_off; uint64_t n_phred;   // NULL: no BAM_QUAL pieces
  const uint64_t* rec_first; uint64_t n_rec;                   // BAM records: every record's first piece [n_rec + 1]
  uint32_t* len; const unsigned char** src;                    // per piece
  const uint64_t* at;                                          // the lengths' exclusive prefix [n_pieces + 1]
  unsigned char* out; uint64_t n_out; uint64_t* rec_off;
  uint64_t* rec_start;                                         // BAM records for the sorter: every record's first byte [n_rec + 1]
};

// lane i: the length and the source of piece i.  A reference outside what it names gives an empty piece (the host clamps them already).
__global__ void __launch_bounds__(256) rc_resolve(RcArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n_pieces) return;
  const lra_rec_piece p = A.piece[i];
  uint64_t n = 0; const unsigned char* s = nullptr;
  const uint64_t idx = p.src >> 32, from = p.src & 0xffffffffu;
  switch (p.kind) {
    case LRA_PIECE_LIT:
      if (p.src <= A.blob_bytes && p.len <= A.blob_bytes - p.src) { n = p.len; s = A.blob + p.src; }
      break;
    case LRA_PIECE_SEQ_FW: case LRA_PIECE_SEQ_RC:
      if (idx < (uint64_t)A.n_reads) {
        const uint64_t b = A.read_off[idx], L = A.read_off[idx + 1] - b;
        if (from <= L) { n = min((uint64_t)p.len, L - from); s = A.strands + b + from + (p.kind == LRA_PIECE_SEQ_RC ? A.rc_base : 0); }
      }
      break;
    case LRA_PIECE_QUAL:
      if (A.qual && idx < (uint64_t)A.n_reads) {
        const uint64_t b = A.qual_off[idx], L = A.qual_off[idx + 1] - b;
        if (from <= L) { n = min((uint64_t)p.len, L - from); s = A.qual + b + from; }
      }
      break;
    case LRA_PIECE_CIGAR:
      if (p.src < A.n_aln) { n = A.cg_off[p.src + 1] - A.cg_off[p.src]; s = A.cg + A.cg_off[p.src]; }
      break;
    case LRA_PIECE_MD:
      if (A.md && p.src < A.n_aln) { n = A.md_off[p.src + 1] - A.md_off[p.src]; s = A.md + A.md_off[p.src]; }
      break;
    case LRA_PIECE_PAIRWISE:
      if (A.pw && p.src < A.n_aln) { n = A.pw_off[p.src + 1] - A.pw_off[p.src]; s = A.pw + A.pw_off[p.src]; }
      break;
    case LRA_PIECE_BAM_CIGAR:
      if (A.bcg && p.src < A.n_aln) { n = 4 * (A.bcg_off[p.src + 1] - A.bcg_off[p.src]); s = (const unsigned char*)(A.bcg + A.bcg_off[p.src]); }
      break;
    case LRA_PIECE_BAM_SEQ:
      if (A.pseq && p.src < A.n_pseq) { n = A.pseq_off[p.src + 1] - A.pseq_off[p.src]; s = A.pseq + A.pseq_off[p.src]; }
      break;
    case LRA_PIECE_BAM_QUAL:
      if (A.phred && p.src < A.n_phred) { n = A.phred_off[p.src + 1] - A.phred_off[p.src]; s = A.phred + A.phred_off[p.src]; }
      break;
    default: break;
  }
  A.len[i] = (uint32_t)n;
  A.src[i] = s;
}

__global__ void __launch_bounds__(256) rc_rec_off(RcArgs A) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r <= A.n_reads) A.rec_off[r] = A.at[A.read_piece[r]];
}

__global__ void __launch_bounds__(256) rc_rec_start(RcArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= A.n_rec) A.rec_start[i] = A.at[A.rec_first[i]];
}

// BAM records, behind the copy: lane i writes record i's block_size, its bytes less the field's own four, at the record's first byte (any alignment: by bytes)
__global__ void __launch_bounds__(256) rc_block_size(RcArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n_rec) return;
  const uint64_t b = A.at[A.rec_first[i]], e = A.at[A.rec_first[i + 1]];
  if (e < b + 4 || e > A.n_out) return;
  const uint32_t v = (uint32_t)(e - b - 4);
  for (int k = 0; k < 4; k++) A.out[b + k] = (unsigned char)(v >> (8 * k));
}

// one wave per chunk of the output bytes (chunk_copy.h)
__global__ void __launch_bounds__(256) rc_copy(RcArgs A) {
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  chunk_copy<RC_CHUNK>(A.out, A.n_out, A.n_pieces, A.at, [&](uint64_t p) { return A.src[p]; }, wave, n_waves, threadIdx.x & 63);
}

inline size_t sz(size_t n, size_t e) { return (n * e + 255) & ~(size_t)255; }
}  // namespace

extern "C" int lra_cigar_text_batch(lra_ctx* ctx, int n_aln, const uint32_t* d_runs, const uint64_t* d_run_off, const int32_t* d_pre_clip, const int32_t* d_suf_clip,
                                    const uint8_t* d_clip_op, lra_cigar_text_result* out) {
  if (!ctx || !out || n_aln < 0 || (n_aln > 0 && !d_run_off)) return LRA_ERR_INVALID;
  memset(out, 0, sizeof(*out));
  out->n_aln = n_aln;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t nA = (size_t)n_aln;
  uint64_t nR = 0;
  if (n_aln) {
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&nR, d_run_off + n_aln, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  }
  if (nR && !d_runs) return LRA_ERR_INVALID;
  const bool clips = n_aln && (d_pre_clip || d_suf_clip);
  CgArgs A; memset(&A, 0, sizeof A);
  A.n_aln = n_aln; A.n_runs = nR; A.runs = d_runs; A.run_off = d_run_off; A.pre = d_pre_clip; A.suf = d_suf_clip; A.clip_op = d_clip_op;
  // 1: per run its bytes and their prefix, per alignment the clips' bytes and their prefix, the two totals side by side behind them
  char* w = (char*)lra_ensure(ctx, 1, sz(nR, 1) + sz(nR + 1, 8) + sz(nA, 1) + sz(nA + 1, 8) + 256);
  if (!w) return LRA_ERR_NOMEM;
  A.w = (uint8_t*)w; w += sz(nR, 1);
  uint64_t* T = (uint64_t*)w; w += sz(nR + 1, 8);
  uint8_t* cw = (uint8_t*)w; w += sz(nA, 1);
  uint64_t* Cx = (uint64_t*)w; w += sz(nA + 1, 8);
  uint64_t* d_tot = (uint64_t*)w;
  if (clips) A.cw = cw;
  uint64_t tot[2] = {0, 0};                                  // the runs' bytes, the clips' bytes
  const uint64_t lanes = std::max<uint64_t>(nR, nA + 1);
  if (n_aln) {
    lra_time_begin(ctx, "cigar_text");
    hipLaunchKernelGGL(cg_count, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, A);
    if (lra_exclusive_scan<uint8_t>(ctx, (long)nR, A.w, T)) return LRA_ERR_HIP;
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(d_tot, T + nR, 8, hipMemcpyDeviceToDevice, st));
    if (clips) {
      if (lra_exclusive_scan<uint8_t>(ctx, (long)nA, cw, Cx)) return LRA_ERR_HIP;
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(d_tot + 1, Cx + nA, 8, hipMemcpyDeviceToDevice, st));
    } else LRA_HIP_CHECK(ctx, hipMemsetAsync(d_tot + 1, 0, 8, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(tot, d_tot, 16, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  }
  const uint64_t nT = tot[0] + tot[1];
  // 2: the result -- off, the text (+ 64 bytes: the record stage reads aligned dwords)
  char* r = (char*)lra_ensure(ctx, 2, sz(nA + 1, 8) + sz(nT + 64, 1));
  if (!r) return LRA_ERR_NOMEM;
  A.T = T; A.C = clips ? Cx : nullptr; A.off = (uint64_t*)r; A.text = (unsigned char*)(r + sz(nA + 1, 8)); A.n_text = nT;
  if (n_aln) {
    hipLaunchKernelGGL(cg_emit, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, A);
    lra_time_end(ctx);
  } else LRA_HIP_CHECK(ctx, hipMemsetAsync(A.off, 0, 8, st));
  LRA_HIP_CHECK(ctx, hipGetLastError());
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  out->n_bytes = nT; out->d_off = A.off; out->d_text = (const char*)A.text;
  return LRA_OK;
}

// The records of a batch from its piece table: the text in the context's page-locked record buffer, rec_off[n_reads + 1] in h_rec_off.
int lra_records_assemble(lra_ctx* ctx, const lra_rec_job& J, const char** text, uint64_t* len, uint64_t* h_rec_off, lra_records_device_stats* S) {
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t nP = J.n_pieces, nR = (size_t)J.n_reads;
  if (len) *len = 0;
  if (text) *text = nullptr;
  if (!nP) { for (size_t r = 0; r <= nR; r++) h_rec_off[r] = 0; return LRA_OK; }
  auto wall = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t0 = wall();
  // 30: what the host wrote -- the pieces, every read's first piece, the literal blob (+ 64 bytes: aligned dwords are read)
  const size_t nRec = J.rec_first ? (size_t)J.n_rec : 0;
  char* u = (char*)lra_ensure(ctx, 30, sz(nP, sizeof(lra_rec_piece)) + sz(nR + 1, 8) + sz(J.blob_bytes + 64, 1) + sz(nRec + 1, 8));
  // 31: per piece -- its length, its source, the lengths' prefix; rec_off; the text's bytes
  const bool starts = nRec && J.d_rec_start;
  char* w = (char*)lra_ensure(ctx, 31, sz(nP, 4) + sz(nP, 8) + 2 * sz(nP + 1, 8) + sz(nR + 1, 8) + 256 + (starts ? sz(nRec + 1, 8) : 0));
  if (!u || !w) return LRA_ERR_NOMEM;
  RcArgs A; memset(&A, 0, sizeof A);
  A.n_pieces = nP; A.n_reads = J.n_reads; A.n_aln = J.n_aln;
  A.piece = (const lra_rec_piece*)u; u += sz(nP, sizeof(lra_rec_piece));
  A.read_piece = (const uint64_t*)u; u += sz(nR + 1, 8);
  A.blob = (const unsigned char*)u; A.blob_bytes = J.blob_bytes; u += sz(J.blob_bytes + 64, 1);
  if (nRec) {
    A.rec_first = (const uint64_t*)u; A.n_rec = nRec;
    LRA_HIP_CHECK(ctx, hipMemcpyAsync((void*)A.rec_first, J.rec_first, (nRec + 1) * 8, hipMemcpyHostToDevice, st));
  }
  LRA_HIP_CHECK(ctx, hipMemcpyAsync((void*)A.piece, J.pieces, nP * sizeof(lra_rec_piece), hipMemcpyHostToDevice, st));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync((void*)A.read_piece, J.read_piece, (nR + 1) * 8, hipMemcpyHostToDevice, st));
  if (J.blob_bytes) LRA_HIP_CHECK(ctx, hipMemcpyAsync((void*)A.blob, J.blob, J.blob_bytes, hipMemcpyHostToDevice, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  const double t1 = wall();
  A.strands = (const unsigned char*)J.d_strands; A.read_off = J.d_read_off; A.rc_base = J.rc_base;
  A.qual = (const unsigned char*)J.d_qual; A.qual_off = J.d_qual_off;
  A.cg = (const unsigned char*)J.d_cg; A.cg_off = J.d_cg_off; A.md = (const unsigned char*)J.d_md; A.md_off = J.d_md_off;
  A.pw = (const unsigned char*)J.d_pw; A.pw_off = J.d_pw_off;
  A.bcg = J.d_bcg; A.bcg_off = J.d_bcg_off; A.pseq = J.d_pseq; A.pseq_off = J.d_pseq_off; A.n_pseq = J.n_pseq;
  A.phred = J.d_phred; A.phred_off = J.d_phred_off; A.n_phred = J.n_phred;
  A.len = (uint32_t*)w; w += sz(nP, 4);
  A.src = (const unsigned char**)w; w += sz(nP, 8);
  uint64_t* at = (uint64_t*)w; w += sz(nP + 1, 8);
  A.at = at;
  A.rec_off = (uint64_t*)w; w += sz(nR + 1, 8);
  if (starts) A.rec_start = (uint64_t*)(w + 256);
  uint64_t total = 0;
  hipEvent_t e0, e1, e2;
  LRA_HIP_CHECK(ctx, hipEventCreate(&e0)); LRA_HIP_CHECK(ctx, hipEventCreate(&e1)); LRA_HIP_CHECK(ctx, hipEventCreate(&e2));
  lra_time_begin(ctx, "records_resolve");
  hipLaunchKernelGGL(rc_resolve, dim3((unsigned)((nP + 255) / 256)), dim3(256), 0, st, A);
  if (lra_exclusive_scan<uint32_t>(ctx, (long)nP, A.len, at)) return LRA_ERR_HIP;
  hipLaunchKernelGGL(rc_rec_off, dim3((unsigned)((nR + 1 + 255) / 256)), dim3(256), 0, st, A);
  if (starts) hipLaunchKernelGGL(rc_rec_start, dim3((unsigned)((nRec + 1 + 255) / 256)), dim3(256), 0, st, A);
  lra_time_end(ctx);
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&total, at + nP, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(h_rec_off, A.rec_off, (nR + 1) * 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  // 99: the text
  A.out = (unsigned char*)lra_ensure(ctx, 99, sz(total + 64, 1));
  if (!A.out) return LRA_ERR_NOMEM;
  A.n_out = total;
  if (!J.keep_on_device && ctx->rec_pin_bytes < total) {                            // the page-locked buffer the text lands in: kept, grown with a quarter of headroom
    if (ctx->rec_pin) { (void)hipHostFree(ctx->rec_pin); ctx->rec_pin = nullptr; ctx->rec_pin_bytes = 0; }
    const size_t want = total + total / 4 + 4096;
    if (hipHostMalloc(&ctx->rec_pin, want, hipHostMallocDefault) != hipSuccess) { ctx->rec_pin = nullptr; return lra_set_err(ctx, LRA_ERR_NOMEM, "hipHostMalloc(%zu) failed", want); }
    ctx->rec_pin_bytes = want;
  }
  const double t2 = wall();
  LRA_HIP_CHECK(ctx, hipEventRecord(e0, st));
  if (total) {
    const uint64_t n_chunks = (total + RC_CHUNK - 1) / RC_CHUNK;
    lra_time_begin(ctx, "records_copy");
    hipLaunchKernelGGL(rc_copy, dim3((unsigned)std::min<uint64_t>((n_chunks + 3) / 4, (uint64_t)ctx->num_cu * 32)), dim3(256), 0, st, A);
    if (nRec) hipLaunchKernelGGL(rc_block_size, dim3((unsigned)((nRec + 255) / 256)), dim3(256), 0, st, A);
    lra_time_end(ctx);
  }
  LRA_HIP_CHECK(ctx, hipEventRecord(e1, st));
  if (total && !J.keep_on_device) LRA_HIP_CHECK(ctx, hipMemcpyAsync(ctx->rec_pin, A.out, total, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipEventRecord(e2, st));
  LRA_HIP_CHECK(ctx, hipGetLastError());
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  if (S) {
    float ms = 0;
    S->ms_upload += t1 - t0; S->ms_kernels += t2 - t1;
    if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) { S->ms_copy_kernel = ms; S->ms_kernels += ms; }
    if (hipEventElapsedTime(&ms, e1, e2) == hipSuccess) S->ms_text_copy = ms;
    S->bytes_h2d += nP * sizeof(lra_rec_piece) + (nR + 1) * 8 + J.blob_bytes + (nRec ? (nRec + 1) * 8 : 0);
    S->bytes_d2h += (J.keep_on_device ? 0 : total) + (nR + 1) * 8 + 8;
    S->text_bytes = total; S->n_pieces = nP;
  }
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipEventDestroy(e2);
  if (len) *len = total;
  if (text) *text = J.keep_on_device ? (const char*)A.out : (const char*)ctx->rec_pin;
  if (J.d_rec_start) *J.d_rec_start = A.rec_start;
  return LRA_OK;
}

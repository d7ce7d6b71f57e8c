// lra_amd/csrc/pairwise.hip -- print format 'a' on the device (gfx950): the alignment strings of a batch of alignments (CreateAlignmentStrings,
// Alignment.h:247-331) and the 50-column text Alignment::PrintPairwise (:564-589) prints from them, both straight from the final blocks.
//
// The columns.  Block i of an alignment gives `length` pair columns; behind every block but the last come the net query gap (read characters over '-'),
// the net text gap ('-' over chromosome characters) and the common stretch of the two gaps as pair columns again: length + max(qgap, tgap) columns.  A
// pair column carries '|' or '*' by seqMap equality (so an N against a base is not what MD's upper-case compare says), a gap column ' '.  pw_block cuts a
// block into these four parts and pw_column turns a column of a block into (class, read index, chromosome index); both entry points go through them, so
// the count pass and the emit passes cannot disagree.  Inside a gap the index of the side that has no character is that of its NEXT character: exactly
// the number PrintPairwise prints in front of a row that starts there (first_q / first_t + the non-gap columns before the row), so a row's two numbers
// are one pw_column call on its first column and no pass over the characters.
//
// Shape: count, scan, emit, flat over the batch.  pw_count, a lane per block, writes the block's columns (pw_last: the last block of an alignment has no
// gap behind it); a scan (scan.h) gives every block its first column, P.  lra_alignment_strings_batch: pw_strings, a lane per four columns of the batch,
// finds its block in P (and the block's alignment in block_off) by binary search and stores one dword into each of the three arrays.
// lra_pairwise_text_batch: the text of an alignment of c columns is 46 * ceil(c / 50) + 3 c bytes (a row of n columns: the width-10 number, " q: ", the
// n characters, '\n'; 14 spaces, n characters, '\n'; the number, " t: ", n characters, '\n'; '\n'), so pw_aln and two scans give every alignment its
// bytes and its ROW GROUPS: PW_GROUP_ROWS consecutive rows, one wave each, so a 1 Mb block is 1250 waves and a 10^5-block alignment as many as its
// columns need.  pw_emit: the wave finds its alignment (binary search over the groups' prefix), narrows P to the blocks under its rows, writes the rows'
// characters and headers into an LDS tile laid out with the destination's own misalignment, and copies the tile out in whole aligned dwords (bytes only
// at the two ragged ends).
//
// Limits of the contract.  (1) A block of negative length or a negative gap (blocks that overlap) is outside it: the reference asserts, the pipeline
// makes none, svsig.hip treats them the same way.  Such a length / gap counts as 0 here -- in pw_block, so for count and emit alike: nothing is read
// outside [block i, block i + 1) and nothing written out of range, but the contents differ from the host form's cumulative walk.  (2) A literal '-' in a
// read or a chromosome is outside it too: lra_format_pairwise counts a row's coordinates from the characters (it would skip that base), this file from
// the blocks.
#include "common.h"
#include "scan.h"
#include <algorithm>

namespace {

constexpr int PW_WIDTH = 50;                                 // columns per printed row
constexpr int PW_ROW_FIXED = 46;                             // bytes of a row besides its 3 n characters
constexpr int PW_FULL_ROW = PW_ROW_FIXED + 3 * PW_WIDTH;     // 196
constexpr int PW_GROUP_ROWS = 16;                            // rows per wave of pw_emit (lra_amd/refine.py: PAIRWISE_GROUP_ROWS)
constexpr int PW_TILE_BYTES = PW_GROUP_ROWS * PW_FULL_ROW;   // the LDS tile of a wave: 3136 bytes
constexpr int PW_TILE_WORDS = PW_TILE_BYTES / 4 + 2;         // (+ the destination's misalignment, 0..3 bytes)
enum { PW_PAIR = 0, PW_QGAP = 1, PW_TGAP = 2 };

struct PwBlock { int64_t q0, t0; uint32_t L, nq, nt, nc; };  // pair columns, net query gap, net text gap, common stretch

// B: the block's triple (the next block's behind it unless `last`)
__device__ __forceinline__ PwBlock pw_block(const int32_t* __restrict__ B, bool last) {
  PwBlock r;
  r.q0 = B[0]; r.t0 = B[1];
  const int64_t L = B[2] > 0 ? B[2] : 0;
  r.L = (uint32_t)L; r.nq = r.nt = r.nc = 0;
  if (!last) {
    int64_t qg = (int64_t)B[3] - B[0] - L, tg = (int64_t)B[4] - B[1] - L;
    if (qg < 0) qg = 0;
    if (tg < 0) tg = 0;
    const int64_t c = qg < tg ? qg : tg;
    r.nq = (uint32_t)(qg - c); r.nt = (uint32_t)(tg - c); r.nc = (uint32_t)c;
  }
  return r;
}
__device__ __forceinline__ uint32_t pw_cols(const PwBlock& b) { return b.L + b.nq + b.nt + b.nc; }   // <= max(q1 - q0, t1 - t0) < 2^32

// column k of the block: its class and the read / chromosome index of its character (of the next character on a side that has none here)
__device__ __forceinline__ int pw_column(const PwBlock& b, uint32_t k, int64_t& q, int64_t& t) {
  if (k < b.L) { q = b.q0 + k; t = b.t0 + k; return PW_PAIR; }
  k -= b.L;
  const int64_t q1 = b.q0 + b.L, t1 = b.t0 + b.L;
  if (k < b.nq) { q = q1 + k; t = t1; return PW_QGAP; }
  k -= b.nq;
  if (k < b.nt) { q = q1 + b.nq; t = t1 + k; return PW_TGAP; }
  k -= b.nt;
  q = q1 + b.nq + k; t = t1 + b.nt + k;
  return PW_PAIR;
}

__device__ __forceinline__ int pw_seq_map(unsigned char c) {                // seqMap (SeqUtils.h:7-40) as emit.hip restates it
  switch (c) {
    case 1: case 5: case 'C': case 'c': return 1;
    case 2: case 6: case 'G': case 'g': return 2;
    case 3: case 7: case 'T': case 't': return 3;
    default: return 0;
  }
}
// the three characters of a column; the characters are copied as they are stored
__device__ __forceinline__ void pw_chars(int cls, const unsigned char* __restrict__ R, const unsigned char* __restrict__ G, int64_t q, int64_t t,
                                         unsigned char& qc, unsigned char& ac, unsigned char& tc) {
  if (cls == PW_PAIR) { qc = R[q]; tc = G[t]; ac = pw_seq_map(qc) != pw_seq_map(tc) ? '*' : '|'; }
  else if (cls == PW_QGAP) { qc = R[q]; tc = '-'; ac = ' '; }
  else { qc = '-'; tc = G[t]; ac = ' '; }
}

struct PwArgs {
  int n_aln; uint64_t n_blocks;
  const int32_t* blocks; const uint64_t* block_off;
  const unsigned char* qseq; const uint64_t* q_off; const unsigned char* tseq; const uint64_t* t_off;
  uint32_t* cols; const uint64_t* P;                           // per block: its columns; their exclusive prefix [n_blocks + 1]
  uint64_t* col_off; uint32_t* ref_len;                        // the strings' result (NULL for the text)
  unsigned char* sq; unsigned char* sa; unsigned char* st; uint64_t n_cols;
  uint64_t* tlen; uint64_t* ngrp;                              // per alignment: the text's bytes, its row groups (NULL for the strings)
  const uint64_t* off; const uint64_t* goff;                   // their exclusive prefixes [n_aln + 1]
  unsigned char* text; uint64_t n_text, n_groups;
};

__global__ void __launch_bounds__(256) pw_count(PwArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < A.n_blocks) A.cols[i] = pw_cols(pw_block(A.blocks + 3 * i, i + 1 == A.n_blocks));
}
// an alignment's last block has no gap behind it (pw_count saw the next alignment's first block there)
__global__ void __launch_bounds__(256) pw_last(PwArgs A) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= A.n_aln) return;
  const uint64_t b0 = A.block_off[a], b1 = A.block_off[a + 1];
  if (b1 > b0 && b1 <= A.n_blocks) A.cols[b1 - 1] = pw_cols(pw_block(A.blocks + 3 * (b1 - 1), true));
}

// lane a: what the alignment's columns come to
__global__ void __launch_bounds__(256) pw_aln(PwArgs A) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a > A.n_aln) return;
  const uint64_t b0 = A.block_off[a];
  if (A.col_off) A.col_off[a] = A.P[b0];
  if (a == A.n_aln) return;
  const uint64_t b1 = A.block_off[a + 1];
  if (A.ref_len) A.ref_len[a] = b1 > b0 ? (uint32_t)(A.blocks[3 * (b1 - 1) + 1] + A.blocks[3 * (b1 - 1) + 2]) : 0u;
  if (A.tlen) {
    const uint64_t c = A.P[b1] - A.P[b0], rows = (c + PW_WIDTH - 1) / PW_WIDTH;
    A.tlen[a] = PW_ROW_FIXED * rows + 3 * c;
    A.ngrp[a] = (rows + PW_GROUP_ROWS - 1) / PW_GROUP_ROWS;
  }
}

// lane i: columns [4 i, 4 i + 4) of the batch, one dword into each array
__global__ void __launch_bounds__(256) pw_strings(PwArgs A) {
  const uint64_t j0 = 4 * ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
  if (j0 >= A.n_cols) return;
  uint64_t b = 0, e = A.n_blocks - 1;                          // the first block whose columns end behind j0
  while (b < e) { const uint64_t mid = (b + e) >> 1; if (A.P[mid + 1] <= j0) b = mid + 1; else e = mid; }
  int a = 0, ae = A.n_aln - 1;                                 // its alignment: the first whose blocks end behind b
  while (a < ae) { const int mid = (a + ae) >> 1; if (A.block_off[mid + 1] <= b) a = mid + 1; else ae = mid; }
  uint64_t pb = A.P[b], pe = A.P[b + 1], bend = A.block_off[a + 1];
  PwBlock blk = pw_block(A.blocks + 3 * b, b + 1 == bend);
  const unsigned char* R = A.qseq + A.q_off[a];
  const unsigned char* G = A.tseq + A.t_off[a];
  const int n = (int)min((uint64_t)4, A.n_cols - j0);
  uint32_t wq = 0, wa = 0, wt = 0;
  for (int k = 0; k < n; k++) {
    const uint64_t j = j0 + k;
    if (j >= pe) {
      do { b++; pb = pe; pe = A.P[b + 1]; } while (j >= pe);   // (j < n_cols = P[n_blocks]: b stays a block)
      if (b >= bend) {
        do { a++; bend = A.block_off[a + 1]; } while (b >= bend);
        R = A.qseq + A.q_off[a]; G = A.tseq + A.t_off[a];
      }
      blk = pw_block(A.blocks + 3 * b, b + 1 == bend);
    }
    int64_t q, t;
    const int cls = pw_column(blk, (uint32_t)(j - pb), q, t);
    unsigned char qc, ac, tc;
    pw_chars(cls, R, G, q, t, qc, ac, tc);
    wq |= (uint32_t)qc << (8 * k); wa |= (uint32_t)ac << (8 * k); wt |= (uint32_t)tc << (8 * k);
  }
  if (n == 4) { *(uint32_t*)(A.sq + j0) = wq; *(uint32_t*)(A.sa + j0) = wa; *(uint32_t*)(A.st + j0) = wt; }
  else for (int k = 0; k < n; k++) { A.sq[j0 + k] = (unsigned char)(wq >> (8 * k)); A.sa[j0 + k] = (unsigned char)(wa >> (8 * k)); A.st[j0 + k] = (unsigned char)(wt >> (8 * k)); }
}

// the width(10) number in front of a row
__device__ __forceinline__ void pw_put_w10(unsigned char* p, uint32_t v) {
  for (int k = 9; k >= 0; k--) { p[k] = (v || k == 9) ? (unsigned char)('0' + v % 10u) : (unsigned char)' '; v /= 10u; }
}

// one wave per row group
__global__ void __launch_bounds__(256) pw_emit(PwArgs A) {
  __shared__ uint32_t tile[4][PW_TILE_WORDS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t g = (uint64_t)blockIdx.x * 4 + w;
  bool live = g < A.n_groups;
  unsigned char* dst = nullptr; uint64_t nbytes = 0; uint32_t shift = 0;
  if (live) {
    int a = 0, ae = A.n_aln - 1;                               // the group's alignment: the first whose groups end behind g
    while (a < ae) { const int mid = (a + ae) >> 1; if (A.goff[mid + 1] <= g) a = mid + 1; else ae = mid; }
    const uint64_t b0 = A.block_off[a], b1 = A.block_off[a + 1], base = A.P[b0];
    const uint64_t c = A.P[b1] - base, rows = (c + PW_WIDTH - 1) / PW_WIDTH;
    const uint64_t r0 = (g - A.goff[a]) * PW_GROUP_ROWS, r1 = min(rows, r0 + PW_GROUP_ROWS);
    const uint64_t col0 = r0 * PW_WIDTH, col1 = min(c, r1 * PW_WIDTH);
    const uint64_t at = A.off[a] + r0 * PW_FULL_ROW;
    live = r0 < r1 && b1 > b0 && b1 <= A.n_blocks;
    if (live) {
      const int nr = (int)(r1 - r0), ncol = (int)(col1 - col0);
      const int nlast = ncol - PW_WIDTH * (nr - 1);            // the columns of the group's last row (every row in front of it is full)
      nbytes = (uint64_t)PW_ROW_FIXED * nr + 3 * (uint64_t)ncol;
      live = at + nbytes <= A.off[a + 1] && A.off[a + 1] <= A.n_text;   // (nothing is written past the alignment's text, whatever the counts say)
      if (live) {
        dst = A.text + at;
        shift = (uint32_t)((uintptr_t)dst & 3);
        unsigned char* s = (unsigned char*)tile[w] + shift;
        const unsigned char* R = A.qseq + A.q_off[a];
        const unsigned char* G = A.tseq + A.t_off[a];
        // the blocks under the group's columns: [blo, bhi]
        uint64_t blo = b0, e = b1 - 1;
        while (blo < e) { const uint64_t mid = (blo + e) >> 1; if (A.P[mid + 1] <= base + col0) blo = mid + 1; else e = mid; }
        uint64_t bhi = blo; e = b1 - 1;
        while (bhi < e) { const uint64_t mid = (bhi + e) >> 1; if (A.P[mid + 1] <= base + col1 - 1) bhi = mid + 1; else e = mid; }
        auto column = [&](uint64_t j, int64_t& q, int64_t& t) {   // column j of the alignment
          uint64_t b = blo, be = bhi;
          while (b < be) { const uint64_t mid = (b + be) >> 1; if (A.P[mid + 1] <= base + j) b = mid + 1; else be = mid; }
          const PwBlock blk = pw_block(A.blocks + 3 * b, b + 1 == b1);
          return pw_column(blk, (uint32_t)(base + j - A.P[b]), q, t);
        };
        for (int x = lane; x < ncol; x += 64) {
          int64_t q, t;
          const int cls = column(col0 + x, q, t);
          unsigned char qc, ac, tc;
          pw_chars(cls, R, G, q, t, qc, ac, tc);
          const int rr = x / PW_WIDTH, cc = x - rr * PW_WIDTH, n = rr == nr - 1 ? nlast : PW_WIDTH;
          unsigned char* p = s + rr * PW_FULL_ROW + 14 + cc;
          p[0] = qc; p[15 + n] = ac; p[2 * (15 + n)] = tc;
        }
        if (lane < nr) {                                       // the row's frame: the two numbers, the labels, the line ends
          const int n = lane == nr - 1 ? nlast : PW_WIDTH;
          int64_t q, t;
          (void)column(col0 + (uint64_t)lane * PW_WIDTH, q, t);
          unsigned char* p = s + lane * PW_FULL_ROW;
          pw_put_w10(p, (uint32_t)q); p[10] = ' '; p[11] = 'q'; p[12] = ':'; p[13] = ' '; p[14 + n] = '\n';
          p += 15 + n;
          for (int k = 0; k < 14; k++) p[k] = ' ';
          p[14 + n] = '\n';
          p += 15 + n;
          pw_put_w10(p, (uint32_t)t); p[10] = ' '; p[11] = 't'; p[12] = ':'; p[13] = ' '; p[14 + n] = '\n'; p[15 + n] = '\n';
        }
      }
    }
  }
  __syncthreads();
  if (!live) return;
  const unsigned char* s = (const unsigned char*)tile[w] + shift;
  const uint64_t head = min(nbytes, (uint64_t)((4 - shift) & 3));
  if ((uint64_t)lane < head) dst[lane] = s[lane];
  const uint64_t nd = (nbytes - head) >> 2, tail = (nbytes - head) & 3;
  uint32_t* d32 = (uint32_t*)(dst + head);
  const uint32_t* s32 = tile[w] + ((shift + head) >> 2);       // (shift + head is 0 or 4: the tile's dwords are the destination's)
  for (uint64_t i = lane; i < nd; i += 64) d32[i] = s32[i];
  if ((uint64_t)lane < tail) dst[head + 4 * nd + lane] = s[head + 4 * nd + lane];
}

inline size_t sz(size_t n, size_t e) { return (n * e + 255) & ~(size_t)255; }

// What both entry points start with: the blocks' columns and their prefix.  101: the small arrays of either call (the results' offsets among them).
int pw_prepare(lra_ctx* ctx, int n_aln, const int32_t* d_blocks, const uint64_t* d_block_off, const char* d_qseq, const uint64_t* d_q_off, const char* d_tseq,
               const uint64_t* d_t_off, PwArgs& A, char** rest) {
  hipStream_t st = ctx->stream;
  const size_t nA = (size_t)n_aln;
  uint64_t nB = 0;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&nB, d_block_off + n_aln, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  memset(&A, 0, sizeof A);
  A.n_aln = n_aln; A.n_blocks = nB; A.blocks = d_blocks; A.block_off = d_block_off;
  A.qseq = (const unsigned char*)d_qseq; A.q_off = d_q_off; A.tseq = (const unsigned char*)d_tseq; A.t_off = d_t_off;
  char* w = (char*)lra_ensure(ctx, 101, sz(nB, 4) + sz(nB + 1, 8) + 4 * sz(nA + 1, 8) + sz(nA, 4) + 256);
  if (!w) return LRA_ERR_NOMEM;
  A.cols = (uint32_t*)w; w += sz(nB, 4);
  uint64_t* P = (uint64_t*)w; w += sz(nB + 1, 8);
  A.P = P;
  *rest = w;
  lra_time_begin(ctx, "pairwise_count");                       // (closed by the caller behind pw_aln and its scans)
  if (nB) {
    hipLaunchKernelGGL(pw_count, dim3((unsigned)((nB + 255) / 256)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(pw_last, dim3((unsigned)((nA + 255) / 256)), dim3(256), 0, st, A);
  }
  if (lra_exclusive_scan<uint32_t>(ctx, (long)nB, A.cols, P)) return LRA_ERR_HIP;
  return LRA_OK;
}

bool pw_bad_args(lra_ctx* ctx, int n_aln, const void* a, const void* b, const void* c, const void* d, const void* e, const void* f, const void* out) {
  return !ctx || !out || n_aln < 0 || (n_aln > 0 && (!a || !b || !c || !d || !e || !f));
}
}  // namespace

extern "C" int lra_alignment_strings_batch(lra_ctx* ctx, int n_aln, const int32_t* d_blocks, const uint64_t* d_block_off, const char* d_qseq,
                                           const uint64_t* d_q_off, const int32_t* d_q_len, const char* d_tseq, const uint64_t* d_t_off,
                                           lra_aln_strings_result* out) {
  (void)d_q_len;
  if (pw_bad_args(ctx, n_aln, d_blocks, d_block_off, d_qseq, d_q_off, d_tseq, d_t_off, out)) return LRA_ERR_INVALID;
  memset(out, 0, sizeof(*out));
  out->n_aln = n_aln;
  if (n_aln == 0) return LRA_OK;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t nA = (size_t)n_aln;
  PwArgs A; char* w = nullptr;
  int rc = pw_prepare(ctx, n_aln, d_blocks, d_block_off, d_qseq, d_q_off, d_tseq, d_t_off, A, &w);
  if (rc) return rc;
  A.col_off = (uint64_t*)w; w += sz(nA + 1, 8);
  A.ref_len = (uint32_t*)w;
  hipLaunchKernelGGL(pw_aln, dim3((unsigned)((nA + 1 + 255) / 256)), dim3(256), 0, st, A);
  lra_time_end(ctx);
  uint64_t total = 0;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&total, A.P + A.n_blocks, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  // 102: the three strings (+ 64 bytes each, so that whoever reads them may read aligned dwords)
  const size_t each = sz(total + 64, 1);
  char* r = (char*)lra_ensure(ctx, 102, 3 * each);
  if (!r) return LRA_ERR_NOMEM;
  A.sq = (unsigned char*)r; A.sa = A.sq + each; A.st = A.sa + each; A.n_cols = total;
  if (total) {
    lra_time_begin(ctx, "pairwise_strings");
    hipLaunchKernelGGL(pw_strings, dim3((unsigned)(((total + 3) / 4 + 255) / 256)), dim3(256), 0, st, A);
    lra_time_end(ctx);
  }
  LRA_HIP_CHECK(ctx, hipGetLastError());
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  out->n_cols = total; out->d_col_off = A.col_off; out->d_ref_len = A.ref_len;
  out->d_q = (const char*)A.sq; out->d_a = (const char*)A.sa; out->d_t = (const char*)A.st;
  return LRA_OK;
}

extern "C" int lra_pairwise_text_batch(lra_ctx* ctx, int n_aln, const int32_t* d_blocks, const uint64_t* d_block_off, const char* d_qseq,
                                       const uint64_t* d_q_off, const int32_t* d_q_len, const char* d_tseq, const uint64_t* d_t_off,
                                       lra_pairwise_text_result* out) {
  (void)d_q_len;
  if (pw_bad_args(ctx, n_aln, d_blocks, d_block_off, d_qseq, d_q_off, d_tseq, d_t_off, out)) return LRA_ERR_INVALID;
  memset(out, 0, sizeof(*out));
  out->n_aln = n_aln;
  if (n_aln == 0) return LRA_OK;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t nA = (size_t)n_aln;
  PwArgs A; char* w = nullptr;
  int rc = pw_prepare(ctx, n_aln, d_blocks, d_block_off, d_qseq, d_q_off, d_tseq, d_t_off, A, &w);
  if (rc) return rc;
  A.tlen = (uint64_t*)w; w += sz(nA + 1, 8);
  A.ngrp = (uint64_t*)w; w += sz(nA + 1, 8);
  uint64_t* off = (uint64_t*)w; w += sz(nA + 1, 8);
  uint64_t* goff = (uint64_t*)w;
  hipLaunchKernelGGL(pw_aln, dim3((unsigned)((nA + 1 + 255) / 256)), dim3(256), 0, st, A);
  if (lra_exclusive_scan<uint64_t>(ctx, (long)nA, A.tlen, off) || lra_exclusive_scan<uint64_t>(ctx, (long)nA, A.ngrp, goff)) return LRA_ERR_HIP;
  lra_time_end(ctx);
  uint64_t total = 0, nG = 0;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&total, off + nA, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&nG, goff + nA, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  if ((nG + 3) / 4 > 0x7fffffffull) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_pairwise_text_batch: %llu row groups", (unsigned long long)nG);
  // 103: the text (+ 64 bytes: the record stage reads aligned dwords)
  A.text = (unsigned char*)lra_ensure(ctx, 103, sz(total + 64, 1));
  if (!A.text) return LRA_ERR_NOMEM;
  A.off = off; A.goff = goff; A.n_text = total; A.n_groups = nG;
  if (nG) {
    lra_time_begin(ctx, "pairwise_emit");
    hipLaunchKernelGGL(pw_emit, dim3((unsigned)((nG + 3) / 4)), dim3(256), 0, st, A);
    lra_time_end(ctx);
  }
  LRA_HIP_CHECK(ctx, hipGetLastError());
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  out->n_bytes = total; out->d_off = off; out->d_text = (const char*)A.text;
  return LRA_OK;
}

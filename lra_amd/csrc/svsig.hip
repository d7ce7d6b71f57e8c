// lra_amd/csrc/svsig.hip -- the SV signatures of a batch of alignments (Alignment::Printsvsig, Alignment.h:336-411; opts.Printsvsig / opts.svsigLen,
// Options.h:69-70) on the device (gfx950).
//
// Printsvsig walks the final blocks of an alignment.  With q / t the end of block b in the read / the chromosome and qg / tg the bases up to block b + 1,
// the common part c = min(qg, tg) is taken off both; what is left on one side is the gap's net length, and the gap sits in front of the c common
// columns.  A net query gap above svsigLen is one INS signature {t, t, qg, read[q, q + qg)}, otherwise a net text gap above it one DEL signature
// {t, t + tg - 1, tg, text[t, t + tg)}.  A pair with a negative gap (the reference asserts) gives nothing.
//
// Shape: flat over the batch's block pairs -- pair i is (block i, block i + 1) of the concatenated block list, so an alignment of 10^5 blocks is 10^5
// lanes like everything else.  sv_count writes a flag and the sequence bytes per pair, sv_cut clears the pair behind every alignment's last block (it
// would join two alignments), two scans (scan.h) give every pair its signature index and sequence offset, and sig_off[a] is the first of them at
// block_off[a].  sv_emit writes the records, sv_copy the sequences: the OUTPUT bytes are cut into pieces of SV_PIECE, one wave per piece, which finds
// the signatures under its piece (the records are in sequence order) and copies a byte per lane -- sources and destinations have every alignment
// mod 16, and a 50 kb deletion is 49 waves, not one.  The host reads three numbers: the batch's block count, then the two totals in one copy.
#include "common.h"
#include "scan.h"

namespace {

constexpr int SV_PIECE = 1024;                               // output bytes per wave of sv_copy (16 per lane); refine.py mirrors it for the tests' shapes

struct SvArgs {
  int n_aln; int32_t min_len;
  uint64_t n_blocks;
  const int32_t* blocks; const uint64_t* block_off;
  const unsigned char* qseq; const uint64_t* q_off;
  const unsigned char* tseq; const uint64_t* t_off;
  uint8_t* flag; uint32_t* bytes;                            // per pair
  const uint64_t* sig_idx; const uint64_t* seq_at;           // their exclusive prefixes [n_blocks + 1]
  uint64_t n_sig, n_seq;
  uint64_t* sig_off; lra_svsig_rec* rec; unsigned char* seq; // the result
};

// the net gap behind block i of the flat list: its length (0: no signature) and kind; q / t = the block's end
__device__ __forceinline__ uint32_t sv_gap(const int32_t* __restrict__ B, uint64_t i, int32_t min_len, int& kind, int64_t& q, int64_t& t) {
  const int32_t* b = B + 3 * i;
  const int64_t len = b[2];
  q = (int64_t)b[0] + len; t = (int64_t)b[1] + len;
  int64_t qg = (int64_t)b[3] - q, tg = (int64_t)b[4] - t;
  kind = LRA_SV_INS;
  if (qg < 0 || tg < 0) return 0;
  const int64_t c = qg < tg ? qg : tg;
  qg -= c; tg -= c;
  if (qg > min_len) return (uint32_t)qg;
  kind = LRA_SV_DEL;
  return tg > min_len ? (uint32_t)tg : 0u;
}

__global__ void __launch_bounds__(256) sv_count(SvArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n_blocks) return;
  uint32_t n = 0;
  if (i + 1 < A.n_blocks) { int kind; int64_t q, t; n = sv_gap(A.blocks, i, A.min_len, kind, q, t); }
  A.flag[i] = n ? 1 : 0;
  A.bytes[i] = n;
}

// the last block of an alignment has no pair: what sv_count wrote there paired it with the next alignment's first block
__global__ void __launch_bounds__(256) sv_cut(SvArgs A) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= A.n_aln) return;
  const uint64_t b0 = A.block_off[a], b1 = A.block_off[a + 1];
  if (b1 > b0) { A.flag[b1 - 1] = 0; A.bytes[b1 - 1] = 0; }
}

// lane i: the record of pair i, when it has one, and sig_off[i] of alignment i (i = n_aln: the total)
__global__ void __launch_bounds__(256) sv_emit(SvArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= (uint64_t)A.n_aln) A.sig_off[i] = A.sig_idx[A.block_off[i]];
  if (i >= A.n_blocks || !A.flag[i]) return;
  const uint64_t s = A.sig_idx[i];
  if (s >= A.n_sig) return;                                  // (nothing is written past the result, whatever the counts say)
  int lo = 0, hi = A.n_aln - 1;                              // the alignment of block i: the first whose blocks end behind it
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (A.block_off[mid + 1] <= i) lo = mid + 1; else hi = mid; }
  int kind; int64_t q, t;
  lra_svsig_rec r;
  r.len = sv_gap(A.blocks, i, A.min_len, kind, q, t);
  r.seq_off = A.seq_at[i]; r.t_start = (uint32_t)t; r.block = (uint32_t)(i - A.block_off[lo]); r.kind = (uint32_t)kind;
  A.rec[s] = r;
}

// one wave per piece of the output bytes
__global__ void __launch_bounds__(64) sv_copy(SvArgs A) {
  const int lane = threadIdx.x;
  const uint64_t n_pieces = (A.n_seq + SV_PIECE - 1) / SV_PIECE;
  for (uint64_t p = blockIdx.x; p < n_pieces; p += gridDim.x) {
    const uint64_t lo = p * SV_PIECE, hi = min(lo + (uint64_t)SV_PIECE, A.n_seq);
    uint64_t s = 0, e = A.n_sig - 1;                         // the first signature whose bytes end behind lo
    while (s < e) { const uint64_t mid = (s + e) >> 1; if (A.rec[mid].seq_off + A.rec[mid].len <= lo) s = mid + 1; else e = mid; }
    int a = 0, ah = A.n_aln - 1;                             // its alignment: the first whose signatures end behind s
    while (a < ah) { const int mid = (a + ah) >> 1; if (A.sig_off[mid + 1] <= s) a = mid + 1; else ah = mid; }
    for (; s < A.n_sig; s++) {
      const lra_svsig_rec r = A.rec[s];
      if (r.seq_off >= hi) break;
      while (A.sig_off[a + 1] <= s) a++;
      const int32_t* b = A.blocks + 3 * (A.block_off[a] + r.block);
      const unsigned char* src = r.kind == LRA_SV_INS ? A.qseq + A.q_off[a] + ((int64_t)b[0] + b[2]) : A.tseq + A.t_off[a] + r.t_start;
      const uint64_t from = max(lo, r.seq_off), to = min(hi, r.seq_off + r.len);
      src += from - r.seq_off;
      for (uint64_t o = from + lane; o < to; o += 64) A.seq[o] = src[o - from];
    }
  }
}

}  // namespace

extern "C" int lra_sv_signatures_batch(lra_ctx* ctx, int n_aln, const int32_t* d_blocks, const uint64_t* d_block_off, const char* d_qseq, const uint64_t* d_q_off,
                                       const int32_t* d_q_len, const char* d_tseq, const uint64_t* d_t_off, int32_t min_len, lra_svsig_result* out) {
  (void)d_q_len;
  if (!ctx || !out || n_aln < 0 || min_len < 0 || (n_aln > 0 && (!d_blocks || !d_block_off || !d_qseq || !d_q_off || !d_tseq || !d_t_off))) return LRA_ERR_INVALID;
  memset(out, 0, sizeof(*out));
  out->n_aln = n_aln;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t nA = (size_t)n_aln;
  auto sz = [](size_t n, size_t e) { return (n * e + 255) & ~(size_t)255; };
  uint64_t nB = 0;
  if (n_aln) {
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&nB, d_block_off + n_aln, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  }
  SvArgs A; memset(&A, 0, sizeof A);
  A.n_aln = n_aln; A.min_len = min_len; A.n_blocks = nB; A.blocks = d_blocks; A.block_off = d_block_off;
  A.qseq = (const unsigned char*)d_qseq; A.q_off = d_q_off; A.tseq = (const unsigned char*)d_tseq; A.t_off = d_t_off;
  uint64_t tot[2] = {0, 0};                                  // signatures, sequence bytes
  uint64_t* sig_idx = nullptr; uint64_t* seq_at = nullptr;
  if (nB) {
    // 188: per pair -- the flags, the bytes and their two prefixes, the totals side by side behind them
    char* w = (char*)lra_ensure(ctx, 188, sz(nB, 1) + sz(nB, 4) + 2 * sz(nB + 1, 8) + 256);
    if (!w) return LRA_ERR_NOMEM;
    A.flag = (uint8_t*)w; w += sz(nB, 1);
    A.bytes = (uint32_t*)w; w += sz(nB, 4);
    sig_idx = (uint64_t*)w; w += sz(nB + 1, 8);
    seq_at = (uint64_t*)w; w += sz(nB + 1, 8);
    uint64_t* d_tot = (uint64_t*)w;
    A.sig_idx = sig_idx; A.seq_at = seq_at;
    lra_time_begin(ctx, "svsig");
    hipLaunchKernelGGL(sv_count, dim3((unsigned)((nB + 255) / 256)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(sv_cut, dim3((unsigned)((nA + 255) / 256)), dim3(256), 0, st, A);
    if (lra_exclusive_scan<uint8_t>(ctx, (long)nB, A.flag, sig_idx)) return LRA_ERR_HIP;
    if (lra_exclusive_scan<uint32_t>(ctx, (long)nB, A.bytes, seq_at)) return LRA_ERR_HIP;
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(d_tot, sig_idx + nB, 8, hipMemcpyDeviceToDevice, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(d_tot + 1, seq_at + nB, 8, hipMemcpyDeviceToDevice, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(tot, d_tot, 16, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  }
  // 189: the result -- sig_off, the records, the sequences
  char* r = (char*)lra_ensure(ctx, 189, sz(nA + 1, 8) + sz(tot[0], sizeof(lra_svsig_rec)) + sz(tot[1], 1) + 256);
  if (!r) return LRA_ERR_NOMEM;
  A.n_sig = tot[0]; A.n_seq = tot[1];
  A.sig_off = (uint64_t*)r; r += sz(nA + 1, 8);
  A.rec = (lra_svsig_rec*)r; r += sz(tot[0], sizeof(lra_svsig_rec));
  A.seq = (unsigned char*)r;
  if (nB) {
    const uint64_t lanes = std::max<uint64_t>(nB, nA + 1);
    hipLaunchKernelGGL(sv_emit, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, A);
    if (tot[1]) {
      const uint64_t n_pieces = (tot[1] + SV_PIECE - 1) / SV_PIECE;
      hipLaunchKernelGGL(sv_copy, dim3((unsigned)std::min<uint64_t>(n_pieces, (uint64_t)ctx->num_cu * 64)), dim3(64), 0, st, A);
    }
    lra_time_end(ctx);
  } else LRA_HIP_CHECK(ctx, hipMemsetAsync(A.sig_off, 0, (nA + 1) * 8, st));
  LRA_HIP_CHECK(ctx, hipGetLastError());
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  out->n_sig = tot[0]; out->n_seq_bytes = tot[1];
  out->d_sig_off = A.sig_off; out->d_sig = A.rec; out->d_seq = (const char*)A.seq;
  return LRA_OK;
}

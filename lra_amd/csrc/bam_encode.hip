// lra_amd/csrc/bam_encode.hip -- the long fields of BAM records (SAM/BAM specification 4.2) made on the device (gfx950): an alignment's CIGAR as BAM ops, ranges
// of bases as 4-bit codes, ranges of quality strings as phred bytes.  Each is flat over the batch and written once into a staging array of its own; the BAM
// form of the device record stage (map_output.hip: lra_map_records_device_bam) points pieces at the three arrays and records.hip's copy pass assembles them.
//
// CIGAR (lra_bam_cigar_batch).  One lane per run: (len << 4) | {0 1 2 3} for = X I D becomes (len << 4) | {7 8 1 2}.  Offsets are in ops.  With clips an
// alignment's ops are its runs with an S / H op on either side where the clip is positive, placed as lra_cigar_text_batch places their text: a scan of the
// clips' counts gives C, run x of alignment a lands at x + C[a] + (the leading clip's op), and the lane looks its alignment up by binary search.
//
// SEQ (lra_bam_pack_seq_batch) and QUAL (lra_bam_phred_batch).  The OUTPUT is cut into chunks of 4 KiB, one wave each, by chunk_copy.h's walk: the wave finds
// the first range under its chunk and makes the ranges' parts that lie in it.  A lane writes an aligned output dword: of SEQ from the 8 source bytes under it,
// read as the two or three aligned dwords around them, through a 256-byte code table in LDS; of QUAL from the 4 source bytes, less 33 each.  The ragged ends
// of a part, and the last dword of a range of SEQ whose 8 bases are not all there, go by bytes.
#include "common.h"
#include "chunk_copy.h"
#include "scan.h"
#include <algorithm>

namespace {

constexpr int BAM_CHUNK = 4096;                               // output bytes per wave of the two packers

inline size_t sz(size_t n, size_t e) { return (n * e + 255) & ~(size_t)255; }
constexpr size_t FRONT = 256;                                // bytes in front of a staging array (its 256-byte alignment; nothing is written there)

// growable device buffer i of the context's BAM staging (contents not kept on growth)
void* bam_room(lra_ctx* ctx, int i, size_t bytes) {
  if (ctx->bam_buf[i] && ctx->bam_bytes[i] >= bytes) return ctx->bam_buf[i];
  if (ctx->bam_buf[i]) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(ctx->bam_buf[i]); ctx->bam_buf[i] = nullptr; ctx->bam_bytes[i] = 0; }
  const size_t want = bytes + bytes / 4 + 4096;
  void* p = nullptr;
  if (hipMalloc(&p, want) != hipSuccess) { lra_set_err(ctx, LRA_ERR_NOMEM, "hipMalloc(%zu) failed", want); return nullptr; }
  ctx->bam_buf[i] = p; ctx->bam_bytes[i] = want;
  return p;
}

// ---- CIGAR ------------------------------------------------------------------------------------------------------------------------------------------
struct BcArgs {
  int n_aln; uint64_t n_runs;
  const uint32_t* runs; const uint64_t* run_off;
  const int32_t* pre; const int32_t* suf; const uint8_t* clip_op;   // NULL: no clips / 'S'
  uint8_t* cw; const uint64_t* C;                              // per alignment its clips' ops; their exclusive prefix [n_aln + 1] (both NULL without clips)
  uint64_t* off; uint32_t* ops; uint64_t n_ops;                // the result
};

__device__ __forceinline__ uint32_t bam_op_of(uint32_t run) {
  const uint32_t op = run & 15u;
  return (run & ~15u) | (op < 4u ? ((0x2187u >> (4 * op)) & 15u) : op);   // = X I D -> 7 8 1 2
}
__device__ __forceinline__ uint32_t bam_clip_of(int32_t len, const uint8_t* clip_op, uint64_t a) {
  return ((uint32_t)len << 4) | ((clip_op && clip_op[a] == 'H') ? 5u : 4u);
}

__global__ void __launch_bounds__(256) bc_count(BcArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (uint64_t)A.n_aln) A.cw[i] = (uint8_t)(((A.pre && A.pre[i] > 0) ? 1 : 0) + ((A.suf && A.suf[i] > 0) ? 1 : 0));
}

// lane i: the op of run i, and off[i] + the clips of alignment i (i = n_aln: the total)
__global__ void __launch_bounds__(256) bc_emit(BcArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= (uint64_t)A.n_aln) {
    const uint64_t at = A.run_off[i] + (A.C ? A.C[i] : 0);
    A.off[i] = at;
    if (A.C && i < (uint64_t)A.n_aln) {
      const int32_t p = A.pre ? A.pre[i] : 0, s = A.suf ? A.suf[i] : 0;
      const uint64_t end = A.run_off[i + 1] + A.C[i + 1];
      if (p > 0 && at < A.n_ops) A.ops[at] = bam_clip_of(p, A.clip_op, i);
      if (s > 0 && end >= 1 && end <= A.n_ops) A.ops[end - 1] = bam_clip_of(s, A.clip_op, i);
    }
  }
  if (i >= A.n_runs) return;
  uint64_t at = i;
  if (A.C) {
    int lo = 0, hi = A.n_aln - 1;                              // the alignment of run i: the first whose runs end behind it
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (A.run_off[mid + 1] <= i) lo = mid + 1; else hi = mid; }
    at += A.C[lo] + ((A.pre && A.pre[lo] > 0) ? 1 : 0);
  }
  if (at < A.n_ops) A.ops[at] = bam_op_of(A.runs[i]);          // (nothing is written past the result, whatever the counts say)
}

// ---- SEQ and QUAL -----------------------------------------------------------------------------------------------------------------------------------
// n bytes at dst by one wave: dst in aligned dwords from dword_at(k) (the dword of bytes k .. k + 3), bytes from byte_at(k) in front of the first aligned
// dword and behind the last
template <typename DW, typename BY>
__device__ __forceinline__ void wave_make(unsigned char* dst, uint64_t n, int lane, DW dword_at, BY byte_at) {
  const uint64_t head = min(n, (uint64_t)((4 - ((uintptr_t)dst & 3)) & 3));
  if ((uint64_t)lane < head) dst[lane] = byte_at((uint64_t)lane);
  const uint64_t nd = (n - head) >> 2;
  uint32_t* d32 = (uint32_t*)(dst + head);
  for (uint64_t i = lane; i < nd; i += 64) d32[i] = dword_at(head + 4 * i);
  const uint64_t tail = (n - head) & 3, t0 = head + 4 * nd;
  if ((uint64_t)lane < tail) dst[t0 + lane] = byte_at(t0 + lane);
}

// the 8 bytes at s as two dwords, from the aligned dwords that hold them (each holds a byte of s[0, 8), so it lies in that byte's page)
__device__ __forceinline__ void load8(const unsigned char* s, uint32_t& w0, uint32_t& w1) {
  const uint32_t sh = (uint32_t)((uintptr_t)s & 3) * 8;
  const uint32_t* q = (const uint32_t*)((uintptr_t)s & ~(uintptr_t)3);
  const uint32_t d0 = q[0], d1 = q[1];
  if (sh == 0) { w0 = d0; w1 = d1; }
  else { const uint32_t d2 = q[2]; w0 = (d0 >> sh) | (d1 << (32 - sh)); w1 = (d1 >> sh) | (d2 << (32 - sh)); }
}
__device__ __forceinline__ uint32_t load4(const unsigned char* s) {
  const uint32_t sh = (uint32_t)((uintptr_t)s & 3) * 8;
  const uint32_t* q = (const uint32_t*)((uintptr_t)s & ~(uintptr_t)3);
  return sh == 0 ? q[0] : (q[0] >> sh) | (q[1] << (32 - sh));
}

// seq_nt16_table as the BAM records use it: "=ACMGRSVTWYHKDBN" in either case -> 0 .. 15, anything else 15
__device__ __forceinline__ uint8_t nt16_of(int c) {
  const int u = (c >= 'a' && c <= 'z') ? c - 32 : c;
  uint8_t code = 15;
#pragma unroll
  for (int k = 0; k < 16; k++) if (u == "=ACMGRSVTWYHKDBN"[k]) code = (uint8_t)k;
  return code;
}

struct SqArgs {
  uint64_t n; const lra_bam_seq_range* range; const unsigned char* src; uint64_t src_bytes;
  uint64_t* cnt; const uint64_t* at;                           // bytes per range; their exclusive prefix [n + 1]
  unsigned char* out; uint64_t n_out;
};
__device__ __forceinline__ bool sq_inside(const SqArgs& A, const lra_bam_seq_range& r) { return r.off <= A.src_bytes && r.len <= A.src_bytes - r.off; }

__global__ void __launch_bounds__(256) sq_count(SqArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < A.n) A.cnt[i] = (A.range[i].len + 1) >> 1;
}

__global__ void __launch_bounds__(256) sq_pack(SqArgs A) {
  __shared__ uint8_t code[256];
  code[threadIdx.x] = nt16_of((int)threadIdx.x);
  __syncthreads();
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const int lane = threadIdx.x & 63;
  chunk_walk<BAM_CHUNK>(A.n_out, A.n, A.at, wave, n_waves, [&](uint64_t p, uint64_t b, uint64_t end, uint64_t lo, uint64_t hi) {
    const lra_bam_seq_range r = A.range[p];
    const bool ok = sq_inside(A, r);                           // (a range that leaves the array is never read: its bases are N)
    const unsigned char* s = A.src + (ok ? r.off : 0);
    const uint64_t from = max(lo, b), to = min(hi, end), j0 = from - b;   // byte j of the range holds bases 2j and 2j + 1
    auto byte_at = [&](uint64_t k) -> unsigned char {
      const uint64_t x = 2 * (j0 + k);
      const uint32_t hiN = ok ? code[s[x]] : 15u, loN = x + 1 < r.len ? (ok ? code[s[x + 1]] : 15u) : 0u;
      return (unsigned char)((hiN << 4) | loN);
    };
    auto dword_at = [&](uint64_t k) -> uint32_t {
      const uint64_t x = 2 * (j0 + k);
      if (!ok || x + 8 > r.len) return (uint32_t)byte_at(k) | ((uint32_t)byte_at(k + 1) << 8) | ((uint32_t)byte_at(k + 2) << 16) | ((uint32_t)byte_at(k + 3) << 24);
      uint32_t w0, w1;
      load8(s + x, w0, w1);
      auto two = [&](uint32_t w) -> uint32_t {                 // 4 bases -> 2 bytes, the first base in the high nibble of the low byte
        return ((uint32_t)code[w & 255u] << 4) | (uint32_t)code[(w >> 8) & 255u] | ((uint32_t)code[(w >> 16) & 255u] << 12) | ((uint32_t)code[w >> 24] << 8);
      };
      return two(w0) | (two(w1) << 16);
    };
    wave_make(A.out + from, to - from, lane, dword_at, byte_at);
  });
}

struct PhArgs {
  uint64_t n; const lra_bam_qual_req* req; int n_reads;
  const unsigned char* qual; const uint64_t* qual_off;         // NULL: no read has qualities
  uint32_t* cnt; const uint64_t* at;
  unsigned char* out; uint64_t n_out;
};

__global__ void __launch_bounds__(256) ph_count(PhArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < A.n) A.cnt[i] = A.req[i].len;
}

__global__ void __launch_bounds__(256) ph_make(PhArgs A) {
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const int lane = threadIdx.x & 63;
  chunk_walk<BAM_CHUNK>(A.n_out, A.n, A.at, wave, n_waves, [&](uint64_t p, uint64_t b, uint64_t end, uint64_t lo, uint64_t hi) {
    const lra_bam_qual_req r = A.req[p];
    const unsigned char* s = nullptr;                          // the request's first character, when [pos, pos + len) lies inside a string that is not "*"
    if (A.qual && r.read < (uint32_t)A.n_reads) {
      const uint64_t q0 = A.qual_off[r.read], L = A.qual_off[r.read + 1] - q0;
      if ((uint64_t)r.pos + r.len <= L && !(L == 1 && A.qual[q0] == '*')) s = A.qual + q0 + r.pos;
    }
    const uint64_t from = max(lo, b), to = min(hi, end), j0 = from - b;
    auto byte_at = [&](uint64_t k) -> unsigned char { return s ? (unsigned char)(s[j0 + k] - 33) : (unsigned char)0xff; };
    auto dword_at = [&](uint64_t k) -> uint32_t {
      if (!s) return 0xffffffffu;
      const uint32_t w = load4(s + j0 + k);
      const uint32_t even = ((w & 0x00ff00ffu) + 0x00df00dfu) & 0x00ff00ffu, odd = (((w >> 8) & 0x00ff00ffu) + 0x00df00dfu) & 0x00ff00ffu;
      return even | (odd << 8);                                // every byte - 33 (mod 256)
    };
    wave_make(A.out + from, to - from, lane, dword_at, byte_at);
  });
}

unsigned packer_blocks(lra_ctx* ctx, uint64_t total) {
  const uint64_t n_chunks = (total + BAM_CHUNK - 1) / BAM_CHUNK;
  return (unsigned)std::min<uint64_t>((n_chunks + 3) / 4, (uint64_t)ctx->num_cu * 32);
}
}  // namespace

extern "C" int lra_bam_cigar_batch(lra_ctx* ctx, int n_aln, const uint32_t* d_runs, const uint64_t* d_run_off, const int32_t* d_pre_clip, const int32_t* d_suf_clip,
                                   const uint8_t* d_clip_op, lra_bam_cigar_result* out) {
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
  BcArgs A; memset(&A, 0, sizeof A);
  A.n_aln = n_aln; A.n_runs = nR; A.runs = d_runs; A.run_off = d_run_off; A.pre = d_pre_clip; A.suf = d_suf_clip; A.clip_op = d_clip_op;
  uint64_t nClip = 0;
  lra_time_begin(ctx, "bam_cigar");
  if (clips) {                                                 // scratch 0 (dead at return): the clips' counts and their prefix
    char* w = (char*)lra_scratch(ctx, 0, sz(nA, 1) + sz(nA + 1, 8));
    if (!w) return LRA_ERR_NOMEM;
    A.cw = (uint8_t*)w;
    uint64_t* Cx = (uint64_t*)(w + sz(nA, 1));
    hipLaunchKernelGGL(bc_count, dim3((unsigned)((nA + 255) / 256)), dim3(256), 0, st, A);
    if (lra_exclusive_scan<uint8_t>(ctx, (long)nA, A.cw, Cx)) return LRA_ERR_HIP;
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&nClip, Cx + nA, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    A.C = Cx;
  }
  const uint64_t nO = nR + nClip;
  uint64_t* off = (uint64_t*)bam_room(ctx, 0, sz(nA + 1, 8));
  char* r = (char*)bam_room(ctx, 1, FRONT + sz(nO, 4) + 64);
  if (!off || !r) return LRA_ERR_NOMEM;
  A.off = off; A.ops = (uint32_t*)(r + FRONT); A.n_ops = nO;
  if (n_aln) {
    const uint64_t lanes = std::max<uint64_t>(nR, nA + 1);
    hipLaunchKernelGGL(bc_emit, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, A);
  } else LRA_HIP_CHECK(ctx, hipMemsetAsync(off, 0, 8, st));
  lra_time_end(ctx);
  LRA_HIP_CHECK(ctx, hipGetLastError());
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  out->n_ops = nO; out->d_off = off; out->d_ops = A.ops;
  return LRA_OK;
}

extern "C" int lra_bam_pack_seq_batch(lra_ctx* ctx, uint64_t n, const lra_bam_seq_range* d_ranges, const uint8_t* d_src, uint64_t src_bytes,
                                      lra_bam_bytes_result* out) {
  if (!ctx || !out || (n && !d_ranges) || (src_bytes && !d_src)) return LRA_ERR_INVALID;
  memset(out, 0, sizeof(*out));
  out->n = n;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  SqArgs A; memset(&A, 0, sizeof A);
  A.n = n; A.range = d_ranges; A.src = d_src; A.src_bytes = src_bytes;
  uint64_t* at = (uint64_t*)bam_room(ctx, 2, sz(n + 1, 8));
  if (!at) return LRA_ERR_NOMEM;
  uint64_t total = 0;
  lra_time_begin(ctx, "bam_pack_seq");
  if (n) {
    A.cnt = (uint64_t*)lra_scratch(ctx, 0, sz(n, 8));
    if (!A.cnt) return LRA_ERR_NOMEM;
    hipLaunchKernelGGL(sq_count, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A);
    if (lra_exclusive_scan<uint64_t>(ctx, (long)n, A.cnt, at)) return LRA_ERR_HIP;
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&total, at + n, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  } else LRA_HIP_CHECK(ctx, hipMemsetAsync(at, 0, 8, st));
  char* r = (char*)bam_room(ctx, 3, FRONT + sz(total, 1) + 64);
  if (!r) return LRA_ERR_NOMEM;
  A.at = at; A.out = (unsigned char*)(r + FRONT); A.n_out = total;
  if (total) hipLaunchKernelGGL(sq_pack, dim3(packer_blocks(ctx, total)), dim3(256), 0, st, A);
  lra_time_end(ctx);
  LRA_HIP_CHECK(ctx, hipGetLastError());
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  out->n_bytes = total; out->d_off = at; out->d_data = A.out;
  return LRA_OK;
}

extern "C" int lra_bam_phred_batch(lra_ctx* ctx, uint64_t n, const lra_bam_qual_req* d_req, int n_reads, const char* d_qual, const uint64_t* d_qual_off,
                                   lra_bam_bytes_result* out) {
  if (!ctx || !out || (n && !d_req) || n_reads < 0 || (d_qual && !d_qual_off)) return LRA_ERR_INVALID;
  memset(out, 0, sizeof(*out));
  out->n = n;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  PhArgs A; memset(&A, 0, sizeof A);
  A.n = n; A.req = d_req; A.n_reads = n_reads; A.qual = (const unsigned char*)d_qual; A.qual_off = d_qual_off;
  uint64_t* at = (uint64_t*)bam_room(ctx, 4, sz(n + 1, 8));
  if (!at) return LRA_ERR_NOMEM;
  uint64_t total = 0;
  lra_time_begin(ctx, "bam_phred");
  if (n) {
    A.cnt = (uint32_t*)lra_scratch(ctx, 0, sz(n, 4));
    if (!A.cnt) return LRA_ERR_NOMEM;
    hipLaunchKernelGGL(ph_count, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A);
    if (lra_exclusive_scan<uint32_t>(ctx, (long)n, A.cnt, at)) return LRA_ERR_HIP;
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&total, at + n, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  } else LRA_HIP_CHECK(ctx, hipMemsetAsync(at, 0, 8, st));
  char* r = (char*)bam_room(ctx, 5, FRONT + sz(total, 1) + 64);
  if (!r) return LRA_ERR_NOMEM;
  A.at = at; A.out = (unsigned char*)(r + FRONT); A.n_out = total;
  if (total) hipLaunchKernelGGL(ph_make, dim3(packer_blocks(ctx, total)), dim3(256), 0, st, A);
  lra_time_end(ctx);
  LRA_HIP_CHECK(ctx, hipGetLastError());
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  out->n_bytes = total; out->d_off = at; out->d_data = A.out;
  return LRA_OK;
}

extern "C" int lra_bam_set_cigar_limit(lra_ctx* ctx, int ops) {
  if (!ctx || ops < 0 || ops > 65535) return LRA_ERR_INVALID;
  ctx->bam_cigar_limit = ops ? ops : 65535;
  return LRA_OK;
}

// lra_amd/csrc/input_bam.hip -- BGZF inflate and BAM record decoding on the device: the kernels behind the BAM steps of lra_reads_next_batch_device
// (input_device.hip drives them) and the inflate stage functions lra_bgzf_inflate_batch / lra_bgzf_inflate_host.
//
//   bgzf_inflate   one wave per BGZF member: lane 0 runs bgzf.h's decoder with its Huffman tables in LDS (1.3 KiB per wave), then the wave computes the
//                  CRC-32 of the member's output (a slice per lane, the slices' CRCs combined as zlib's crc32_combine does) -> a status per member
//   bam_frame      one lane walks the chain of block_size fields of a step's decompressed bytes: the records' starts (a serial dependency)
//   bam_count      a lane per record: validates it (block_size >= 32; name, CIGAR, SEQ and QUAL inside it; the name NUL-terminated), applies
//                  flagRemove, counts its kept bytes (bases, qualities, name, aux)                                    -> exclusive scans
//   bam_emit       a wave per kept record: bases (4-bit codes through "=ACMGRSVTWYHKDBN"), qualities +33 (one NUL slot per record), the name, the aux bytes,
//                  and its entry of the step's record table -- the layout the FASTQ steps produce, so that one batch stage serves both
#include "common.h"
#include "reads_state.h"
#include "zsource.h"
#include "bam_kernels.h"
#include "bgzf.h"

namespace {

constexpr int WAVES = 4;

__global__ void __launch_bounds__(64 * WAVES) bgzf_inflate(int n, const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                           const uint64_t* __restrict__ out_off, uint8_t* out, int32_t* __restrict__ status) {
  __shared__ lra_inflate_tables tabs[WAVES];
  __shared__ uint32_t crc_tab[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) crc_tab[i] = lra_crc32_table_entry((uint32_t)i);
  __syncthreads();
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long b = (long)blockIdx.x * WAVES + w;
  if (b >= n) return;
  const uint64_t i0 = in_off[b], o0 = out_off[b];
  const uint64_t ilen = in_off[b + 1] - i0, olen = out_off[b + 1] - o0;
  int rc = LRA_BGZF_OK;
  uint32_t expect = 0;
  if (lane == 0) {
    const uint8_t* src = in + i0;
    uint32_t total = 0, cdata = 0;
    if (lra_bgzf_member(src, ilen, &total, &cdata) != 1 || total != ilen) rc = LRA_BGZF_ERR_HEADER;
    else if (lra_le32(src + total - 4) != olen || olen > 65536) rc = LRA_BGZF_ERR_ISIZE;
    else {
      uint32_t produced = 0;
      rc = lra_inflate_raw(src + cdata, total - cdata - 8, out + o0, (uint32_t)olen, tabs[w], &produced);
      if (!rc && produced != olen) rc = LRA_BGZF_ERR_SIZE;
      expect = lra_le32(src + total - 8);
    }
  }
  rc = __shfl(rc, 0);
  expect = (uint32_t)__shfl((int)expect, 0);
  if (rc) { if (lane == 0) status[b] = rc; return; }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // lane 0's output, read by the whole wave
  const uint64_t slice = (olen + 63) / 64, lo = lane * slice < olen ? lane * slice : olen, hi = lo + slice < olen ? lo + slice : olen;
  uint32_t part = 0;
  if (hi > lo) part = lra_crc32_shift(lra_crc32_update(0, out + o0 + lo, hi - lo, crc_tab), olen - hi);
  for (int d = 32; d > 0; d >>= 1) part ^= (uint32_t)__shfl_xor((int)part, d);
  if (lane == 0) status[b] = part == expect ? LRA_BGZF_OK : LRA_BGZF_ERR_CRC;
}

__device__ inline uint32_t ld32(const uint8_t* p) { return p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
__device__ inline uint32_t ld16(const uint8_t* p) { return p[0] | ((uint32_t)p[1] << 8); }

__global__ void bam_frame(const uint8_t* __restrict__ d, uint64_t start, uint64_t len, uint64_t* __restrict__ rec_pos, uint64_t cap, uint64_t* __restrict__ out) {
  if (threadIdx.x || blockIdx.x) return;
  uint64_t p = start, n = 0, bad = 0, bad_bs = 0;
  while (p + 4 <= len && n < cap) {
    const uint32_t bs = ld32(d + p);
    if (bs < 32) { bad = 1; bad_bs = bs; break; }
    if (p + 4 + bs > len) break;
    rec_pos[n++] = p;
    p += 4 + (uint64_t)bs;
  }
  out[0] = n; out[1] = p; out[2] = bad; out[3] = bad_bs;
}

struct BamFields { uint32_t bs, l_name, n_cig, flag; int32_t l_seq; uint64_t fixed; bool ok; };
__device__ inline BamFields bam_fields(const uint8_t* p) {
  BamFields f;
  f.bs = ld32(p);
  const uint8_t* r = p + 4;
  f.l_name = r[8]; f.n_cig = ld16(r + 12); f.flag = ld16(r + 14); f.l_seq = (int32_t)ld32(r + 16);
  f.fixed = 32 + (uint64_t)f.l_name + 4ull * f.n_cig + (f.l_seq < 0 ? 0 : ((uint64_t)f.l_seq + 1) / 2 + (uint64_t)f.l_seq);
  f.ok = f.l_seq >= 0 && f.l_name >= 1 && f.fixed <= f.bs && r[32 + f.l_name - 1] == 0;
  return f;
}

__global__ void bam_count(const uint8_t* __restrict__ d, const uint64_t* __restrict__ rec_pos, uint64_t n, uint32_t flag_remove, uint32_t* __restrict__ c_keep,
                          uint32_t* __restrict__ c_seq, uint32_t* __restrict__ c_qual, uint32_t* __restrict__ c_name, uint32_t* __restrict__ c_aux,
                          unsigned long long* __restrict__ first_bad) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t* p = d + rec_pos[i];
  const BamFields f = bam_fields(p);
  if (!f.ok) {
    atomicMin(first_bad, (unsigned long long)i);
    c_keep[i] = c_seq[i] = c_qual[i] = c_name[i] = c_aux[i] = 0;
    return;
  }
  const bool keep = (f.flag & flag_remove) == 0;
  const uint8_t* q = p + 4 + 32 + f.l_name + 4 * f.n_cig + (f.l_seq + 1) / 2;
  const bool hasq = f.l_seq > 0 && q[0] != 0xff;
  c_keep[i] = keep;
  c_seq[i] = keep ? (uint32_t)f.l_seq : 0;
  c_qual[i] = keep && hasq ? (uint32_t)f.l_seq : 0;
  c_name[i] = keep ? f.l_name : 0;
  c_aux[i] = keep ? (uint32_t)(f.bs - f.fixed) : 0;
}

__global__ void __launch_bounds__(64 * WAVES) bam_emit(const uint8_t* __restrict__ d, const uint64_t* __restrict__ rec_pos, uint64_t n,
                                                       const uint32_t* __restrict__ c_keep, const uint64_t* __restrict__ keep_off,
                                                       const uint64_t* __restrict__ seq_off, const uint64_t* __restrict__ qual_off,
                                                       const uint64_t* __restrict__ name_off, const uint64_t* __restrict__ aux_off, char* __restrict__ c_seq,
                                                       char* __restrict__ c_qual, char* __restrict__ c_names, uint8_t* __restrict__ c_aux,
                                                       RecInfo* __restrict__ rec) {
  const uint64_t i = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= n || !c_keep[i]) return;
  const uint8_t* p = d + rec_pos[i];
  const BamFields f = bam_fields(p);
  const uint8_t* r = p + 4;
  const uint8_t* sq = r + 32 + f.l_name + 4 * f.n_cig;
  const uint8_t* q = sq + (f.l_seq + 1) / 2;
  const uint8_t* aux = q + f.l_seq;
  const uint64_t k = keep_off[i], sp = seq_off[i], qp = qual_off[i] + k, np = name_off[i], ap = aux_off[i];
  const uint64_t qlen = qual_off[i + 1] - qual_off[i], alen = aux_off[i + 1] - ap;
  for (int32_t j = lane; j < f.l_seq; j += 64) c_seq[sp + j] = lra_nt16_char(sq[j >> 1] >> ((~j & 1) << 2));
  for (uint64_t j = lane; j < qlen; j += 64) c_qual[qp + j] = (char)(q[j] + 33);
  for (uint32_t j = lane; j < f.l_name; j += 64) c_names[np + j] = (char)r[32 + j];
  for (uint64_t j = lane; j < alen; j += 64) c_aux[ap + j] = aux[j];
  if (lane == 0) {
    c_qual[qp + qlen] = 0;
    RecInfo e;
    e.start = i; e.seq = sp; e.qual = qual_off[i]; e.name = np; e.tok = ap; e.tok_len = (uint32_t)alen; e.flags = qlen > 0;
    rec[k] = e;
  }
}

}  // namespace

void lra_bgzf_launch_inflate(hipStream_t st, int n, const uint8_t* in, const uint64_t* in_off, const uint64_t* out_off, uint8_t* out, int32_t* status) {
  if (n > 0) hipLaunchKernelGGL(bgzf_inflate, dim3((unsigned)((n + WAVES - 1) / WAVES)), dim3(64 * WAVES), 0, st, n, in, in_off, out_off, out, status);
}

void lra_bam_launch_frame(hipStream_t st, const uint8_t* d, uint64_t start, uint64_t len, uint64_t* rec_pos, uint64_t cap, uint64_t* out) {
  hipLaunchKernelGGL(bam_frame, dim3(1), dim3(64), 0, st, d, start, len, rec_pos, cap, out);
}

void lra_bam_launch_count(hipStream_t st, const uint8_t* d, const uint64_t* rec_pos, uint64_t n, uint32_t flag_remove, uint32_t* const cnt[5],
                          unsigned long long* first_bad) {
  if (n) hipLaunchKernelGGL(bam_count, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d, rec_pos, n, flag_remove, cnt[0], cnt[1], cnt[2], cnt[3], cnt[4], first_bad);
}

void lra_bam_launch_emit(hipStream_t st, const uint8_t* d, const uint64_t* rec_pos, uint64_t n, const uint32_t* keep, uint64_t* const off[5], char* c_seq,
                         char* c_qual, char* c_names, uint8_t* c_aux, RecInfo* rec) {
  if (n) hipLaunchKernelGGL(bam_emit, dim3((unsigned)((n + WAVES - 1) / WAVES)), dim3(64 * WAVES), 0, st, d, rec_pos, n, keep, off[0], off[1], off[2], off[3], off[4],
                            c_seq, c_qual, c_names, c_aux, rec);
}

extern "C" int lra_bgzf_inflate_batch(lra_ctx* ctx, int n_blocks, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_out_off, uint8_t* d_out,
                                      int32_t* d_status) {
  if (!ctx || n_blocks < 0 || (n_blocks && (!d_in || !d_in_off || !d_out_off || !d_out || !d_status))) return LRA_ERR_INVALID;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  lra_bgzf_launch_inflate(ctx->stream, n_blocks, d_in, d_in_off, d_out_off, d_out, d_status);
  LRA_HIP_CHECK(ctx, hipGetLastError());
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return LRA_OK;
}

extern "C" int lra_bgzf_inflate_host(int n_blocks, const uint8_t* in, const uint64_t* in_off, const uint64_t* out_off, uint8_t* out, int32_t* status) {
  if (n_blocks < 0 || (n_blocks && (!in || !in_off || !out_off || !out || !status))) return LRA_ERR_INVALID;
  for (int b = 0; b < n_blocks; b++) {
    const uint64_t olen = out_off[b + 1] - out_off[b];
    status[b] = olen > 65536 ? LRA_BGZF_ERR_ISIZE : lra_bgzf_inflate_one(in + in_off[b], in_off[b + 1] - in_off[b], out + out_off[b], olen);
  }
  return LRA_OK;
}

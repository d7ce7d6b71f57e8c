// lra_amd/csrc/pack_strings.hip -- lra_pack_strings_batch: n strings that lie anywhere in one device buffer, packed back to back (gfx950).
//
// The device readers' quality bytes need it (input_device.hip): a step's c_qual holds the strings with one NUL slot behind every record, the record stage
// (lra_map_records_device) wants them back to back with exact ranges.  pk_copy is chunk_copy.h's loop, the one rc_copy runs: the OUTPUT is cut into
// chunks of PK_CHUNK bytes, one wave each; the wave finds the first string under its chunk by binary search in d_dst_off and writes whole aligned dwords,
// each from the two aligned source dwords around it, and single bytes at a string's ragged ends.  What is read of the source: the aligned dwords that
// hold a byte of a source range, nothing else.
#include "common.h"
#include "chunk_copy.h"
#include <algorithm>

namespace {

constexpr int PK_CHUNK = 4096;                               // output bytes per wave of pk_copy; reads_io.py mirrors it for the tests' shapes

__global__ void __launch_bounds__(256) pk_copy(uint64_t n, const unsigned char* __restrict__ src, const uint64_t* __restrict__ pos,
                                               const uint64_t* __restrict__ off, unsigned char* __restrict__ dst, uint64_t total) {
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  chunk_copy<PK_CHUNK>(dst, total, n, off, [&](uint64_t p) { return src + pos[p]; }, wave, n_waves, threadIdx.x & 63);
}

}  // namespace

void lra_pack_strings_launch(hipStream_t st, int num_cu, uint64_t n, const char* d_src, const uint64_t* d_src_pos, const uint64_t* d_dst_off, char* d_dst,
                             uint64_t total) {
  if (!n || !total) return;
  const uint64_t n_chunks = (total + PK_CHUNK - 1) / PK_CHUNK;
  hipLaunchKernelGGL(pk_copy, dim3((unsigned)std::min<uint64_t>((n_chunks + 3) / 4, (uint64_t)std::max(num_cu, 1) * 32)), dim3(256), 0, st, n,
                     (const unsigned char*)d_src, d_src_pos, d_dst_off, (unsigned char*)d_dst, total);
}

extern "C" int lra_pack_strings_batch(lra_ctx* ctx, uint64_t n, const char* d_src, const uint64_t* d_src_pos, const uint64_t* d_dst_off, char* d_dst) {
  if (!ctx || (n && (!d_src_pos || !d_dst_off))) return LRA_ERR_INVALID;
  if (!n) return LRA_OK;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  uint64_t ends[2] = {0, 0};                                 // d_dst_off[0] (must be 0) and the total
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&ends[0], d_dst_off, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&ends[1], d_dst_off + n, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  if (ends[0] != 0) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_pack_strings_batch: d_dst_off[0] is %llu, not 0", (unsigned long long)ends[0]);
  if (ends[1] && (!d_src || !d_dst)) return LRA_ERR_INVALID;
  lra_time_begin(ctx, "pack_strings");
  lra_pack_strings_launch(st, ctx->num_cu, n, d_src, d_src_pos, d_dst_off, d_dst, ends[1]);
  lra_time_end(ctx);
  LRA_HIP_CHECK(ctx, hipGetLastError());
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  return LRA_OK;
}

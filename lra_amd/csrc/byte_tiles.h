// lra_amd/csrc/byte_tiles.h -- what the tiled byte-stream passes of the device readers share (input_device.hip: the read files; genome.hip: the
// genome; zsource.hip: their BGZF steps): the tile shape, the 128-bit load, the workgroup scan, and the growable device / page-locked buffers the readers own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>

namespace {

constexpr int RD_NT = 256, RD_BPT = 16, RD_TILE = RD_NT * RD_BPT;   // a workgroup per 4 KiB tile, 16 bytes per lane (one 128-bit load)
inline uint64_t padded_tiles(uint64_t len) { return std::max<uint64_t>(1, (len + RD_TILE - 1) / RD_TILE) * RD_TILE; }   // the bytes of the tiles over len bytes

__device__ inline void load16(const unsigned char* __restrict__ raw, uint64_t p, unsigned char b[RD_BPT]) {
  const uint4 v = *reinterpret_cast<const uint4*>(raw + p);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < RD_BPT; j++) b[j] = (unsigned char)(w[j >> 2] >> (8 * (j & 3)));
}

// exclusive prefix over the workgroup of one 32-bit count per lane; *tot = the workgroup's sum
__device__ inline uint32_t block_excl(uint32_t v, uint32_t* sh, uint32_t* tot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d); if (lane >= d) inc += o; }
  if (lane == 63) sh[wave] = inc;
  __syncthreads();
  uint32_t wb = 0, t = 0;
#pragma unroll
  for (int w = 0; w < RD_NT / 64; w++) { const uint32_t x = sh[w]; wb += (w < wave) ? x : 0; t += x; }
  __syncthreads();
  *tot = t;
  return wb + inc - v;
}

// C-locale isspace: what `std::stringstream >>` skips
__device__ inline bool is_ws(unsigned char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

}  // namespace

template <typename T> struct DevBuf {
  T* p = nullptr; size_t n = 0;
  bool ensure(size_t want) {                                       // contents NOT kept
    if (want <= n) return true;
    if (p) (void)hipFree(p);
    p = nullptr; n = 0;
    const size_t m = std::max(want, (size_t)4096);
    if (hipMalloc((void**)&p, m * sizeof(T)) != hipSuccess) return false;
    n = m;
    return true;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};
template <typename T> struct PinBuf {
  T* p = nullptr; size_t n = 0;
  bool ensure(size_t want, size_t keep, hipStream_t st) {   // the first `keep` items are kept: the copies into them queued on `st` land first
    if (want <= n) return true;
    if (hipStreamSynchronize(st) != hipSuccess) return false;   // (st may be the null stream)
    const size_t m = std::max({want, n + n / 2, (size_t)(1 << 20) / sizeof(T)});
    T* q = nullptr;
    if (hipHostMalloc((void**)&q, m * sizeof(T), hipHostMallocDefault) != hipSuccess) return false;
    if (keep) memcpy(q, p, keep * sizeof(T));
    if (p) (void)hipHostFree(p);
    p = q; n = m;
    return true;
  }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; n = 0; }
};

// lra_amd/csrc/bam_keys.h -- what lra_bam_sorter (bam_sort.hip) and lra_bam_merger (bam_merge.hip) both run over raw BAM records on the device, so that
// the two order and index records by ONE code: bs_keys, a lane per record, the 64-bit coordinate key with the record's address and length (and the
// validity checks: a record shorter than its fields, a refID outside [-1, n_ref)); bs_span, a wave per record, the per-record fields of the index.
// include/lra_hip.h states the key.  The kernels are TU-local, as scan.h's are.
#pragma once
#include "common.h"

namespace {

struct KeyArgs {
  const uint8_t* data; const uint64_t* start; uint64_t n, ord0, delta;   // delta: data - the lowest allocation
  int n_ref;
  uint64_t* key; uint32_t* ord; uint64_t* addr; uint32_t* len;
  unsigned long long* red; uint32_t* err;                     // red[0] |= key, red[1] &= key
};

__device__ __forceinline__ uint32_t le16(const uint8_t* p) { return p[0] | ((uint32_t)p[1] << 8); }
__device__ __forceinline__ uint32_t le32(const uint8_t* p) { return p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
// the dword at s from the aligned dwords that hold it (the second lies at most 4 bytes behind s + 3: every buffer here has 64 bytes behind its data)
__device__ __forceinline__ uint32_t ld32(const uint8_t* s) {
  const uint32_t sh = (uint32_t)((uintptr_t)s & 3) * 8;
  const uint32_t* q = (const uint32_t*)((uintptr_t)s & ~(uintptr_t)3);
  return sh == 0 ? q[0] : (q[0] >> sh) | (q[1] << (32 - sh));
}

__global__ void __launch_bounds__(256) bs_keys(KeyArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long k_or = 0, k_and = ~0ull;
  if (i < A.n) {
    const uint64_t b = A.start[i] - A.start[0], L = A.start[i + 1] - A.start[i];
    const uint8_t* p = A.data + b;
    uint64_t key = ~0ull;
    bool bad = L < 36 || L > 0xffffffffull || A.start[i + 1] < A.start[i] || A.start[i] < A.start[0] || A.start[i + 1] > A.start[A.n];   // (nothing outside the copy is read)
    if (!bad) {
      const int32_t ref = (int32_t)le32(p + 4), pos = (int32_t)le32(p + 8);
      const uint32_t l_name = p[12], n_cig = le16(p + 16), flag = le16(p + 18);
      bad = (uint64_t)le32(p) + 4 != L || 36 + (uint64_t)l_name + 4ull * n_cig > L || ref < -1 || ref >= A.n_ref;
      key = ((uint64_t)((uint32_t)ref & 0x7fffffffu) << 33) | ((uint64_t)(uint32_t)(pos + 1) << 1) | ((flag >> 4) & 1u);
    }
    if (bad) atomicAdd(A.err, 1u);
    A.key[A.ord0 + i] = key; A.ord[A.ord0 + i] = (uint32_t)(A.ord0 + i);
    A.addr[A.ord0 + i] = A.delta + b; A.len[A.ord0 + i] = (uint32_t)L;
    k_or = key; k_and = key;
  }
  for (int o = 32; o > 0; o >>= 1) { k_or |= __shfl_xor(k_or, o); k_and &= __shfl_xor(k_and, o); }
  if ((threadIdx.x & 63) == 0) { atomicOr(&A.red[0], k_or); atomicAnd(&A.red[1], k_and); }
}

struct Meta { int32_t* ref; int32_t* pos; uint32_t* span; uint32_t* binflag; };   // per sorted record; binflag = bin | (flag & 4 ? 1 << 16 : 0)

__global__ void __launch_bounds__(256) bs_span(uint64_t n, const uint8_t* __restrict__ s, const uint64_t* __restrict__ at, Meta M) {
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const int lane = threadIdx.x & 63;
  for (uint64_t p = wave; p < n; p += n_waves) {
    const uint8_t* c = s + at[p] + 4;
    const uint32_t l_name = c[8], n_cig = le16(c + 12);
    const uint8_t* ops = c + 32 + l_name;
    uint64_t sum = 0;
    for (uint32_t k = lane; k < n_cig; k += 64) {
      const uint32_t op = ld32(ops + 4 * (uint64_t)k);
      if ((0x18du >> (op & 15u)) & 1u) sum += op >> 4;          // M D N = X
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) {
      M.ref[p] = (int32_t)le32(c); M.pos[p] = (int32_t)le32(c + 4);
      M.span[p] = (uint32_t)min(max(sum, (uint64_t)1), (uint64_t)0xffffffffu);
      M.binflag[p] = le16(c + 10) | ((le16(c + 14) & 4u) ? 0x10000u : 0u);
    }
  }
}

}  // namespace

// lra_amd/csrc/chunk_copy.h -- the copy pass of strings that fill an output back to back, cut by OUTPUT bytes: the body of rc_copy (records.hip: the
// pieces of the record text), of pk_copy (pack_strings.hip: lra_pack_strings_batch) and of svt_copy (svsig_text.hip: the bases of the SV signature lines).
// They differ in where a string's bytes come from, which the caller passes in, and svt_copy in that only a window of every string is a copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// n bytes from src to dst by one wave: dst in aligned dwords, each from the two aligned source dwords around it (an aligned dword that holds one byte
// of the source is read whole: it lies in that byte's page), bytes in front of the first aligned dword and behind the last
__device__ __forceinline__ void wave_copy(unsigned char* dst, const unsigned char* src, uint64_t n, int lane) {
  const uint64_t head = min(n, (uint64_t)((4 - ((uintptr_t)dst & 3)) & 3));
  if ((uint64_t)lane < head) dst[lane] = src[lane];
  dst += head; src += head; n -= head;
  const uint64_t nd = n >> 2;
  uint32_t* d32 = (uint32_t*)dst;
  const uint32_t sh = (uint32_t)((uintptr_t)src & 3) * 8;
  const uint32_t* s32 = (const uint32_t*)((uintptr_t)src & ~(uintptr_t)3);
  if (sh == 0) for (uint64_t i = lane; i < nd; i += 64) d32[i] = s32[i];
  else for (uint64_t i = lane; i < nd; i += 64) d32[i] = (s32[i] >> sh) | (s32[i + 1] << (32 - sh));
  const uint64_t tail = n & 3;
  if ((uint64_t)lane < tail) dst[4 * nd + lane] = src[4 * nd + lane];
}

// String p of n_items (n_items >= 1) is out[at[p], at[p + 1]) and comes from src_of(p); at[n_items] = n_out.  The output is cut into chunks of CHUNK
// bytes, one wave each (wave `wave` of `n_waves` takes every n_waves-th chunk): the wave finds the first string under its chunk by binary search and
// copies the strings' parts that lie in it, so a string of 1 MB is 256 waves at CHUNK = 4096 and a chunk of 200-byte strings is one wave.  Empty strings
// cost a step of the walk and nothing else.  src_of is not called for an empty string.
// window(p, b, e), called with string p's range [b, e) of the output when it is not empty, may narrow it to the part src_of(p) fills (its first byte then
// lands at the new b); the bytes outside the window are the caller's to write.  The default copies every string whole.
// The walk itself: body(p, b, end, lo, hi) is called for every non-empty string p = out[b, end) that has bytes in the wave's chunk [lo, hi).  The packers of
// bam_encode.hip, whose bytes are made rather than copied, run it too.
template <int CHUNK, typename Body>
__device__ __forceinline__ void chunk_walk(uint64_t n_out, uint64_t n_items, const uint64_t* __restrict__ at, uint64_t wave, uint64_t n_waves, Body body) {
  const uint64_t n_chunks = (n_out + CHUNK - 1) / CHUNK;
  for (uint64_t c = wave; c < n_chunks; c += n_waves) {
    const uint64_t lo = c * CHUNK, hi = min(lo + (uint64_t)CHUNK, n_out);
    uint64_t p = 0, e = n_items - 1;                           // the first string whose bytes end behind lo
    while (p < e) { const uint64_t mid = (p + e) >> 1; if (at[mid + 1] <= lo) p = mid + 1; else e = mid; }
    uint64_t b = at[p];
    for (; p < n_items && b < hi; p++) {
      const uint64_t end = at[p + 1];
      if (end > b) body(p, b, end, lo, hi);
      b = end;
    }
  }
}

struct chunk_copy_whole { __device__ __forceinline__ void operator()(uint64_t, uint64_t&, uint64_t&) const {} };
template <int CHUNK, typename SrcOf, typename Window = chunk_copy_whole>
__device__ __forceinline__ void chunk_copy(unsigned char* out, uint64_t n_out, uint64_t n_items, const uint64_t* __restrict__ at, SrcOf src_of, uint64_t wave,
                                           uint64_t n_waves, int lane, Window window = Window()) {
  chunk_walk<CHUNK>(n_out, n_items, at, wave, n_waves, [&](uint64_t p, uint64_t b, uint64_t end, uint64_t lo, uint64_t hi) {
    uint64_t wb = b, we = end;
    window(p, wb, we);
    const uint64_t from = max(lo, wb), to = min(hi, we);
    if (to > from) wave_copy(out + from, src_of(p) + (from - wb), to - from, lane);
  });
}

// pk_copy on `st` (pack_strings.hip): lra_pack_strings_batch for a caller that knows total = d_dst_off[n] already; nothing is launched for total = 0
void lra_pack_strings_launch(hipStream_t st, int num_cu, uint64_t n, const char* d_src, const uint64_t* d_src_pos, const uint64_t* d_dst_off, char* d_dst,
                             uint64_t total);

// lra_amd/csrc/sdp_process.h -- what the two ProcessPoint kernels (sdp_process.hip: a wave per read; sdp_process_wg.hip: a workgroup per large read) share: the gap
// cost w(), wave-level reductions and broadcasts, the cooperative searches and the growth of a stack / Block out of the read's pool.  Device code with internal
// linkage, as it had inside the one file; sdp_points.hip takes pwl_w for the gap-cost table.
#pragma once
#include "sdp.h"

namespace lra_sdp {
namespace {

// w(i, j) = -PWL_w(|j - i| + 1)   (SubRountine.h:101-129).  upper_bound over STOPS[0..24) as a count of constants <= x.
// Every visit of ProcessPoint evaluates this a handful of times and a wave runs them one after the other, so it is written for few instructions: the count of
// stops below 1000 in nine compares, one division between 1000 and 9999, five compares beyond; 32-bit conversions wherever the values fit (the reference's
// (long)(float) and (float)(long) give the same numbers there: both truncate / round the same value).
__device__ __forceinline__ float pwl_w(const float* slope, const float* inter, int c1, int c2, long long i, long long j) {
  const long long x = (j > i ? j - i : i - j) + 1;
  if (x <= 2) return x == 1 ? 0.f : -0.f;
  int b; float xf;
  if (x <= 0x7fffffffLL) {
    const int xs = (int)x;
    if (xs < 1000) b = 1 + (xs >= 5) + (xs >= 10) + (xs >= 20) + (xs >= 40) + (xs >= 80) + (xs >= 100) + (xs >= 200) + (xs >= 300) + (xs >= 500);
    else if (xs < 10000) b = 10 + xs / 1000;                              // stops 1000, 2000, ..., 9000
    else b = 19 + (xs >= 15000) + (xs >= 20000) + (xs >= 30000) + (xs >= 40000) + (xs >= 50000);
    xf = (float)xs;
  } else { b = 24; xf = (float)x; }
  const float f = slope[b - 1] * xf + inter[b - 1];
  if (f > -2.0e9f && f < 2.0e9f) {
    int pen = (int)f;
    if (pen >= c1 && pen < c2) pen = c1;
    else if (pen > c2) pen = c2;
    return -(float)pen;
  }
  long long pen = (long long)f;
  if (pen >= c1 && pen < c2) pen = c1;
  else if (pen > c2) pen = c2;
  return -(float)pen;
}

// The same through a table: -w(i, j) for |j - i| + 1 < n as 16-bit integers in LDS (every penalty is an integer: PWL_w truncates), made once per call by
// k_pen_table with pwl_w itself.  A visit evaluates w ten times and more; from the table that is one LDS read instead of ~50 instructions and two reads.
__device__ __forceinline__ float pwl_w_tab(const short* tab, int n, const float* slope, const float* inter, int c1, int c2, long long i, long long j) {
  const long long d = j > i ? j - i : i - j;
  if (d < (long long)n) { const int xi = (int)d; return xi == 0 ? 0.f : -(float)(int)tab[xi]; }   // (x == 1: w returns +0, SubRountine.h:125)
  return pwl_w(slope, inter, c1, c2, i, j);
}
// a + w(x, e) > b + w(y, e) -- the comparison Maximization / FindBoundary make (SubRountine.h:253, :292, :299) -- with the two table reads issued together (one LDS
// round trip instead of two: the wave walks these one after the other)
__device__ __forceinline__ bool pwl_beats(const short* tab, int n, const float* slope, const float* inter, int c1, int c2, float a, long long x, float b, long long y, long long e) {
  const long long d1 = e > x ? e - x : x - e, d2 = e > y ? e - y : y - e;
  const bool in1 = d1 < (long long)n, in2 = d2 < (long long)n;
  const int x1 = in1 ? (int)d1 : 0, x2 = in2 ? (int)d2 : 0;
  const int p1 = tab[x1], p2 = tab[x2];
  const float w1 = in1 ? (x1 == 0 ? 0.f : -(float)p1) : pwl_w(slope, inter, c1, c2, x, e);
  const float w2 = in2 ? (x2 == 0 ? 0.f : -(float)p2) : pwl_w(slope, inter, c1, c2, y, e);
  return a + w1 > b + w2;
}

// The maximum of a float over the 64 lanes, wave-uniform: four row shifts (a row = 16 lanes; lanes with nothing shifted in keep -inf), the two row broadcasts, lane 63.
__device__ __forceinline__ float wave_max_f32(float v) {
  constexpr int NEG_INF = (int)0xff800000u;
  int x = __float_as_int(v);
#define LRA_DPP_MAX(ctrl_, rmask_) x = __float_as_int(fmaxf(__int_as_float(x), __int_as_float(__builtin_amdgcn_update_dpp(NEG_INF, x, (ctrl_), (rmask_), 0xf, false))))
  LRA_DPP_MAX(0x111, 0xf);   // row_shr:1
  LRA_DPP_MAX(0x112, 0xf);   // row_shr:2
  LRA_DPP_MAX(0x114, 0xf);   // row_shr:4
  LRA_DPP_MAX(0x118, 0xf);   // row_shr:8      (lane 15 of a row: the row's maximum)
  LRA_DPP_MAX(0x142, 0xa);   // row_bcast:15   (rows 1 and 3 take the row before them)
  LRA_DPP_MAX(0x143, 0xc);   // row_bcast:31   (rows 2 and 3 take lane 31)
#undef LRA_DPP_MAX
  return __int_as_float(__builtin_amdgcn_readlane(x, 63));
}
__device__ __forceinline__ int rl_i(int v, int src) { return __builtin_amdgcn_readlane(v, src); }           // src must be wave-uniform
__device__ __forceinline__ float rl_f(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }
__device__ __forceinline__ long long rl_ll(long long v, int src) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(v & 0xffffffffLL), src), hi = (unsigned)__builtin_amdgcn_readlane((int)(v >> 32), src);
  return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ long long shfl_ll(long long v, int src) {
  const int lo = __shfl((int)(v & 0xffffffffLL), src), hi = __shfl((int)(v >> 32), src);
  return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

// Wave-uniform values (every lane computes the same number): moved to scalar registers.  The sparse DP's workgroup kernel is almost entirely uniform control
// (one visit = a serial walk the whole wave follows); left in vector registers its state overflows the 128 a wave of a 1024-thread block may hold, and a reload from
// scratch waits behind every pending store of the walk (vector memory completes in order).  SGPRs spill into VGPR lanes instead: no memory.
__device__ __forceinline__ int u_i(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t u_u(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ float u_f(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ long long u_ll(long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(v & 0xffffffffLL)), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ int2 u_i2(int2 v) { return make_int2(u_i(v.x), u_i(v.y)); }
__device__ __forceinline__ uint2 u_u2(uint2 v) { return make_uint2(u_u(v.x), u_u(v.y)); }

// The literal binary search  `while (count > 0) { step = count / 2; it = first + step; if (pred(it)) { first = it + 1; count -= step + 1; }
// else count = step; }`  (FindBoundary :245-254, UPPERbound :209-219), six levels per memory round: lane t = 1..63 evaluates the
// predicate at the probe the search would make after taking the decisions spelled by t's bits; the wave then walks the 63 answers.
template <typename Pred>
__device__ __forceinline__ unsigned coop_search(unsigned first, unsigned count, int lane, Pred pred) {
  while (count > 0) {
    unsigned f = first, c = count;
    bool valid = lane >= 1;
    if (valid) {
      const int depth = 31 - __clz(lane);
      for (int d = depth - 1; d >= 0; --d) {
        if (c == 0) { valid = false; break; }
        const unsigned step = c / 2, it = f + step;
        if ((lane >> d) & 1) { f = it + 1; c -= step + 1; } else c = step;
      }
    }
    const bool p = (valid && c > 0) ? pred(f + c / 2) : false;
    const unsigned long long m = __ballot(p);
    unsigned t = 1;
    while (t < 64 && count > 0) {
      const unsigned step = count / 2, it = first + step;
      const unsigned bit = (unsigned)((m >> t) & 1);
      if (bit) { first = it + 1; count -= step + 1; } else count = step;
      t = 2 * t + bit;
    }
  }
  return first;
}

// FindValueInBlock's UPPERbound (:205-221) over Block, the same six levels per round.  The search ends at its right boundary, and the right boundary is the
// position of its most recent probe that came out false (or the end of the list): that probe's lane still holds the pair, so Block[lo].first comes with the
// search instead of costing one more dependent load.  Returns lo; *x = Block[lo].x when lo < count.
__device__ __forceinline__ unsigned coop_upper_block(const int2* B, unsigned count0, int i1, int lane, int* x) {
  unsigned first = 0, count = count0;
  int bx = -1;
  while (count > 0) {
    unsigned f = first, c = count;
    bool valid = lane >= 1;
    if (valid) {
      const int depth = 31 - __clz(lane);
      for (int d = depth - 1; d >= 0; --d) {
        if (c == 0) { valid = false; break; }
        const unsigned step = c / 2, it = f + step;
        if ((lane >> d) & 1) { f = it + 1; c -= step + 1; } else c = step;
      }
    }
    int2 pr = make_int2(0, 0);
    const bool live = valid && c > 0;
    if (live) pr = B[f + c / 2];
    const bool p = live && i1 >= pr.y;
    const unsigned long long m = __ballot(p);
    unsigned t = 1;
    int lastFalse = -1;
    while (t < 64 && count > 0) {
      const unsigned step = count / 2, it = first + step;
      const unsigned bit = (unsigned)((m >> t) & 1);
      if (bit) { first = it + 1; count -= step + 1; } else { count = step; lastFalse = (int)t; }
      t = 2 * t + bit;
    }
    if (lastFalse >= 0) bx = __builtin_amdgcn_readlane(pr.x, lastFalse);
  }
  *x = bx;
  return u_u(first);
}

// a stack / Block that is full moves to twice the room in the read's pool (the old room is abandoned)
__device__ bool grow_pairs(int2* pairs, uint32_t& off, int& cap, int used, uint32_t* poolUsed, uint32_t poolPair, uint32_t poolPairs) {
  const uint32_t ncap = 2u * (uint32_t)cap;
  const uint32_t at = atomicAdd(poolUsed, ncap);
  if (at + ncap > poolPairs) return false;
  int2* dst = pairs + poolPair + at; const int2* src = pairs + off;
  for (int k = 0; k < used && k < cap; k++) dst[k] = src[k];
  off = poolPair + at; cap = (int)ncap;
  return true;
}
__device__ bool coop_grow_pairs(int2* pairs, uint32_t& off, int& cap, int used, uint32_t* poolUsed, uint32_t poolPair, uint32_t poolPairs, int lane) {
  const uint32_t ncap = 2u * (uint32_t)cap;
  uint32_t at = 0;
  if (lane == 0) at = atomicAdd(poolUsed, ncap);
  at = (uint32_t)__builtin_amdgcn_readfirstlane((int)at);
  if (at + ncap > poolPairs) return false;
  int2* dst = pairs + poolPair + at; const int2* src = pairs + off;
  for (int k = lane; k < used && k < cap; k += 64) dst[k] = src[k];
  wave_sync();
  off = poolPair + at; cap = (int)ncap;
  return true;
}

}  // namespace
}  // namespace lra_sdp

// w() and the comparison of two candidates inside a ProcessPoint kernel, on its LDS copies of the tables (s_pen, penN, s_slope, s_inter, c1, c2)
#define W(i, j) pwl_w_tab(s_pen, penN, s_slope, s_inter, c1, c2, (i), (j))
#define BEATS(a_, x_, b_, y_, e_) pwl_beats(s_pen, penN, s_slope, s_inter, c1, c2, (a_), (x_), (b_), (y_), (e_))
// A push on the owner's candidate stack / Block list inside the wave-cooperative Maximization of either kernel (oS / oB: the lists, oTop / oBlk: their sizes, ...)
#define SPUSH(val_) do { const int2 v__ = (val_); if (oTop >= oSCap) { if (coop_grow_pairs(pairs, oStkOff, oSCap, oTop, poolUsed, poolPair, poolPairs, lane)) oS = pairs + oStkOff; else ost |= LRA_ST_CAPACITY; } \
                         if (oTop < oSCap) oS[oTop] = v__; oTop++; } while (0)
#define BPUSH(val_) do { const int2 v__ = (val_); if (oBlk >= oBCap) { if (coop_grow_pairs(pairs, oBlkOff, oBCap, oBlk, poolUsed, poolPair, poolPairs, lane)) oB = pairs + oBlkOff; else ost |= LRA_ST_CAPACITY; } \
                         if (oBlk < oBCap) oB[oBlk] = v__; oBlk++; olastB = v__; } while (0)

// lra_amd/csrc/bam_contained.h -- the contained-alignment filter of the reference's call_assembly_SVs/ParseAlignment.py over the framed records of a window
// (bam_pass.h), for the consumers that call variants from a sorted assembly BAM (bam_vcf.hip).  include/lra_hip.h states the rule under lra_bam_vcf.
//
// rule.  Over the records with refID >= 0, in file order: e(i) = pos + 1 + tlen in 64 bits (tlen as stored: lra writes tEnd - tStart).  The first record
// of a run of equal refID is kept; record i is dropped when e(i) <= the largest e of the earlier records of its run (equal ends drop).  The script's
// current_end is that running maximum: a dropped record never exceeds it.
// scan.  A segmented max-scan in scan.h's three phases.  An element is a span of records: the refID of its first and of its last record that takes part,
// the largest e of the trailing run of records with the last one's refID, and whether that run begins inside the span (reset: what stands in front of the
// span does not reach it).  Spans combine associatively, so tiles reduce alone (ct_tile), one lane folds the tile sums behind the carry (ct_parts), and the
// tiles scan again behind their prefix (ct_drop): a record is dropped when the span in front of it ends in its refID with an e at or above its own.
// carry.  The span of everything the pass has delivered is one element; lra_contained::window() computes the next one for the n records it is given and
// commit() takes it when the window is delivered -- a window that is run again with fewer records after a refusal starts from the same carry.
#pragma once
#include "common.h"
#include "bam_rec.h"

namespace {

struct CtSpan { int32_t first, last; int32_t reset, pad; int64_t v; };   // first < 0: no record takes part

__host__ __device__ __forceinline__ CtSpan ct_none() { CtSpan s; s.first = s.last = -1; s.reset = 0; s.pad = 0; s.v = INT64_MIN; return s; }
__host__ __device__ __forceinline__ CtSpan ct_join(const CtSpan& a, const CtSpan& b) {
  if (b.first < 0) return a;
  if (a.first < 0) return b;
  CtSpan s; s.first = a.first; s.last = b.last; s.pad = 0;
  if (b.reset || a.last != b.first) { s.v = b.v; s.reset = 1; }
  else { s.v = a.v > b.v ? a.v : b.v; s.reset = a.reset; }
  return s;
}
// does the record (ref, e) lie inside what span p, in front of it, has seen of its run
__host__ __device__ __forceinline__ bool ct_inside(const CtSpan& p, int32_t ref, int64_t e) { return p.first >= 0 && p.last == ref && e <= p.v; }

constexpr int CT_PER = 8, CT_TILE = 256 * CT_PER;

struct Ct {
  const uint8_t* data; const uint64_t* pos; uint64_t n, limit;   // records at or behind `limit` take no part (a region's chunk ends there)
  CtSpan* part; CtSpan* carry;                                   // part[nb + 1]: the tiles' sums, then their prefixes; carry[0] in, carry[1] out
  uint32_t* drop; uint64_t nb;
};

__device__ __forceinline__ CtSpan ct_record(const Ct& C, uint64_t i) {
  if (i >= C.n) return ct_none();
  const uint64_t at = C.pos[i];
  if (at >= C.limit) return ct_none();
  const uint8_t* p = C.data + at;
  const int32_t ref = (int32_t)le32(p + 4);
  if (ref < 0) return ct_none();
  CtSpan s; s.first = s.last = ref; s.reset = 0; s.pad = 0;
  s.v = (int64_t)(int32_t)le32(p + 8) + 1 + (int64_t)(int32_t)le32(p + 32);
  return s;
}
__device__ __forceinline__ CtSpan ct_shfl_up(const CtSpan& s, int d) {
  CtSpan o; o.first = __shfl_up(s.first, d); o.last = __shfl_up(s.last, d); o.reset = __shfl_up(s.reset, d); o.pad = 0; o.v = (int64_t)__shfl_up((unsigned long long)s.v, d);
  return o;
}
// The block's tile: each lane folds its CT_PER records, the lanes scan.  -> the span of the tile's records in front of this lane's; *total (lane 255): the tile's.
__device__ __forceinline__ CtSpan ct_block_scan(const Ct& C, uint64_t lo, CtSpan* mine, CtSpan* total) {
  __shared__ CtSpan wsum[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  CtSpan own = ct_none();
  for (int k = 0; k < CT_PER; k++) own = ct_join(own, ct_record(C, lo + (uint64_t)threadIdx.x * CT_PER + k));
  CtSpan inc = own;
  for (int d = 1; d < 64; d <<= 1) { const CtSpan o = ct_shfl_up(inc, d); if (lane >= d) inc = ct_join(o, inc); }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  CtSpan ex = ct_shfl_up(inc, 1);
  if (lane == 0) ex = ct_none();
  CtSpan base = ct_none(), tot = ct_none();
  for (int w = 0; w < 4; w++) { if (w < wave) base = ct_join(base, wsum[w]); tot = ct_join(tot, wsum[w]); }
  *mine = own; *total = tot;
  return ct_join(base, ex);
}

__global__ void __launch_bounds__(256) ct_tile(Ct C) {
  CtSpan own, tot;
  (void)ct_block_scan(C, (uint64_t)blockIdx.x * CT_TILE, &own, &tot);
  if (threadIdx.x == 0) C.part[blockIdx.x] = tot;
}
// one lane: the tiles' sums become the spans in front of the tiles, the carry in front of them all; carry[1] = the span behind the last
__global__ void ct_parts(Ct C) {
  if (blockIdx.x || threadIdx.x) return;
  CtSpan run = C.carry[0];
  for (uint64_t b = 0; b < C.nb; b++) { const CtSpan t = C.part[b]; C.part[b] = run; run = ct_join(run, t); }
  C.carry[1] = run;
}
__global__ void __launch_bounds__(256) ct_drop(Ct C) {
  CtSpan own, tot;
  const uint64_t lo = (uint64_t)blockIdx.x * CT_TILE;
  CtSpan run = ct_join(C.part[blockIdx.x], ct_block_scan(C, lo, &own, &tot));
  for (int k = 0; k < CT_PER; k++) {
    const uint64_t i = lo + (uint64_t)threadIdx.x * CT_PER + k;
    if (i >= C.n) break;
    const CtSpan r = ct_record(C, i);
    C.drop[i] = r.first >= 0 && ct_inside(run, r.first, r.v) ? 1u : 0u;
    run = ct_join(run, r);
  }
}

// the filter's state in a consumer of the pass
struct lra_contained {
  Buf<CtSpan> part, carry; Buf<uint32_t> drop;
  bool pending = false;
  void release() { part.release(); carry.release(); drop.release(); }
  // a pass begins: nothing seen
  bool begin(hipStream_t st) {
    if (!carry.ensure(2)) { (void)hipGetLastError(); return false; }
    const CtSpan none[2] = {ct_none(), ct_none()};
    pending = false;
    return hipMemcpyAsync(carry.p, none, sizeof none, hipMemcpyHostToDevice, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
  }
  // drop.p[i] for the window's records [0, n), behind the committed carry; the next carry waits in carry[1]
  bool window(hipStream_t st, const uint8_t* data, const uint64_t* pos, uint64_t n, uint64_t limit) {
    const uint64_t nb = (n + CT_TILE - 1) / CT_TILE;
    if (!part.ensure(nb + 1) || !drop.ensure(n + 1)) { (void)hipGetLastError(); return false; }
    Ct C; C.data = data; C.pos = pos; C.n = n; C.limit = limit; C.part = part.p; C.carry = carry.p; C.drop = drop.p; C.nb = nb;
    if (nb) hipLaunchKernelGGL(ct_tile, dim3((unsigned)nb), dim3(256), 0, st, C);
    hipLaunchKernelGGL(ct_parts, dim3(1), dim3(64), 0, st, C);
    if (nb) hipLaunchKernelGGL(ct_drop, dim3((unsigned)nb), dim3(256), 0, st, C);
    pending = true;
    return hipGetLastError() == hipSuccess;
  }
  void forget() { pending = false; }
  // the window is delivered: its span is the carry (the stream orders this behind the window's kernels and in front of the next window's)
  bool commit(hipStream_t st) {
    if (!pending) return true;
    pending = false;
    return hipMemcpyAsync(carry.p, carry.p + 1, sizeof(CtSpan), hipMemcpyDeviceToDevice, st) == hipSuccess;
  }
};

}  // namespace

// lra_amd/csrc/bam_rec.h -- what the readers of raw BAM records on the device share (bam_view.hip, bam_depth.hip, bam_vcf.hip, bam_svcalls.hip): a record's
// core fields, the walk over its aux block, the test for the CG:B:I form of a long CIGAR and where a record's ops are, the packed SEQ as bases by one wave,
// decimal digits, and the small host helpers of every windowed BAM object, the sorter and the merger with them (event timer, grid sizes, wall clock, the
// growable device array).  The kernels over a window's records that every pass runs -- the check, the region test, the cut -- are bam_pass.h's front.
// The kernels and helpers are TU-local, as scan.h's and bam_keys.h's are.
#pragma once
#include "common.h"
#include "bam_keys.h"
#include <algorithm>
#include <chrono>

namespace {

__device__ __forceinline__ uint64_t le64(const uint8_t* p) { return (uint64_t)le32(p) | ((uint64_t)le32(p + 4) << 32); }
__device__ __forceinline__ int ndig(uint64_t v) { int d = 1; while (v >= 10) { v /= 10; d++; } return d; }
__device__ __forceinline__ int slen(int64_t v) { return v < 0 ? 1 + ndig((uint64_t)(-v)) : ndig((uint64_t)v); }
__device__ __forceinline__ unsigned char* put_u(unsigned char* d, uint64_t v) {
  const int k = ndig(v);
  for (int i = k - 1; i >= 0; i--) { d[i] = (unsigned char)('0' + v % 10); v /= 10; }
  return d + k;
}
__device__ __forceinline__ unsigned char* put_s(unsigned char* d, int64_t v) {
  if (v < 0) { *d++ = '-'; return put_u(d, (uint64_t)(-v)); }
  return put_u(d, (uint64_t)v);
}
// the last index i < n with a[i] <= x (a ascends, a[0] <= x)
__device__ __forceinline__ uint64_t last_le(const uint64_t* __restrict__ a, uint64_t n, uint64_t x) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (a[mid] <= x) lo = mid + 1; else hi = mid; }
  return lo - 1;
}
__device__ __forceinline__ int type_size(uint8_t t) {
  switch (t) { case 'c': case 'C': case 'A': return 1; case 's': case 'S': return 2; case 'i': case 'I': case 'f': return 4; default: return 0; }
}

struct Core { int32_t ref, pos, next_ref, next_pos, tlen; uint32_t bs, l_name, mapq, n_cig, flag, l_seq; uint64_t fixed; };
__device__ __forceinline__ Core core_of(const uint8_t* p) {
  Core c;
  c.bs = le32(p); c.ref = (int32_t)le32(p + 4); c.pos = (int32_t)le32(p + 8); c.l_name = p[12]; c.mapq = p[13]; c.n_cig = le16(p + 16); c.flag = le16(p + 18);
  c.l_seq = le32(p + 20); c.next_ref = (int32_t)le32(p + 24); c.next_pos = (int32_t)le32(p + 28); c.tlen = (int32_t)le32(p + 32);
  c.fixed = 32 + (uint64_t)c.l_name + 4ull * c.n_cig + ((uint64_t)c.l_seq + 1) / 2 + (uint64_t)c.l_seq;
  return c;
}
// what every reader refuses about a record's arithmetic: `len` is the framed length (block_size field included)
__device__ __forceinline__ bool core_ok(const uint8_t* p, const Core& c, uint64_t len, int n_ref) {
  return (uint64_t)c.bs + 4 == len && c.l_name >= 1 && c.fixed <= c.bs && p[36 + c.l_name - 1] == 0 && c.ref >= -1 && c.ref < n_ref;
}
// the core CIGAR at `ops` is <l_seq>S<n>N: the record's real ops are those of its CG:B:I tag, when it has one
__device__ __forceinline__ bool cg_form_at(const uint8_t* ops, const Core& c) {
  return c.n_cig == 2 && le32(ops) == ((c.l_seq << 4) | 4u) && (le32(ops + 4) & 15u) == 3u;
}

// The tag at data[at, end): false when it ends behind `end` or names an unknown type.  *val = its value's offset (B: the first element), *count = elements (B),
// bytes in front of the NUL (Z, H) or 1; *next = the byte behind it.
__device__ __forceinline__ bool tag_at(const uint8_t* d, uint64_t at, uint64_t end, uint8_t* type, uint8_t* sub, uint64_t* val, uint32_t* count, uint64_t* next) {
  if (end - at < 3) return false;
  const uint8_t t = d[at + 2];
  *type = t; *sub = 0; *val = at + 3; *count = 1;
  const int sz = type_size(t);
  if (sz) {
    if (end - at < 3 + (uint64_t)sz) return false;
    *next = at + 3 + sz;
    return true;
  }
  if (t == 'Z' || t == 'H') {
    uint64_t e = at + 3;
    while (e < end && d[e]) e++;
    if (e >= end) return false;
    *count = (uint32_t)(e - (at + 3)); *next = e + 1;
    return true;
  }
  if (t == 'B') {
    if (end - at < 8) return false;
    const uint8_t s = d[at + 3];
    const int es = s == 'A' ? 0 : type_size(s);
    if (!es) return false;
    const uint32_t n = le32(d + at + 4);
    if ((uint64_t)n * es > end - at - 8) return false;
    *sub = s; *val = at + 8; *count = n; *next = at + 8 + (uint64_t)n * es;
    return true;
  }
  return false;
}

// Where record at0's ops are (depth and the variant walk count the same ones): the core CIGAR, or the elements of the CG:B:I tag, wherever it stands in the
// aux block, when the core CIGAR is <l_seq>S<n>N and the record has the tag.  false: the aux block ends inside a tag or names an unknown type in front of it.
__device__ __forceinline__ bool ops_of(const uint8_t* data, uint64_t at0, uint64_t end, const Core& c, uint64_t* ops, uint32_t* n_op) {
  *ops = at0 + 36 + c.l_name; *n_op = c.n_cig;
  if (!cg_form_at(data + *ops, c)) return true;
  uint64_t at = at0 + 4 + c.fixed;
  while (at < end) {
    uint8_t t, s; uint64_t val, next; uint32_t cnt;
    if (!tag_at(data, at, end, &t, &s, &val, &cnt, &next)) return false;
    if (data[at] == 'C' && data[at + 1] == 'G' && t == 'B' && s == 'I') { *ops = val; *n_op = cnt; return true; }
    at = next;
  }
  return true;
}

// n bases of the packed sequence `seq` from base j0 on to dst, by one wave: dst in aligned dwords, each lane two of them (eight bases) from one source
// dword (and the byte behind it when the eight start in a byte's low nibble); bytes in front of the first aligned dword and behind the last whole eight.
// A byte holds its first base in the high nibble: with the nibbles of every byte swapped, nibble m of the source is base m.
__device__ __forceinline__ uint32_t four_bases(uint32_t v) {   // the four nibbles of v's low 16 bits, the first base lowest
  const char* T = "=ACMGRSVTWYHKDBN";
  return (uint32_t)(uint8_t)T[v & 15] | ((uint32_t)(uint8_t)T[(v >> 4) & 15] << 8) | ((uint32_t)(uint8_t)T[(v >> 8) & 15] << 16) | ((uint32_t)(uint8_t)T[(v >> 12) & 15] << 24);
}
__device__ __forceinline__ unsigned char base_at(const uint8_t* seq, uint64_t j) { return (unsigned char)"=ACMGRSVTWYHKDBN"[(seq[j >> 1] >> ((~j & 1) << 2)) & 15]; }
__device__ __forceinline__ void wave_seq(unsigned char* dst, const uint8_t* seq, uint64_t j0, uint64_t n, int lane) {
  const uint64_t head = min(n, (uint64_t)((4 - ((uintptr_t)dst & 3)) & 3));
  if ((uint64_t)lane < head) dst[lane] = base_at(seq, j0 + lane);
  dst += head; j0 += head; n -= head;
  const uint64_t n8 = n >> 3;
  uint32_t* d32 = (uint32_t*)dst;
  for (uint64_t i = lane; i < n8; i += 64) {
    const uint64_t j = j0 + 8 * i;
    const uint8_t* s = seq + (j >> 1);
    uint64_t w = ld32(s);
    if (j & 1) w |= (uint64_t)s[4] << 32;                      // (base j + 7 is the high nibble of s[4]: inside the sequence)
    uint64_t x = ((w & 0x0f0f0f0f0full) << 4) | ((w >> 4) & 0x0f0f0f0f0full);
    if (j & 1) x >>= 4;
    d32[2 * i] = four_bases((uint32_t)x & 0xffffu); d32[2 * i + 1] = four_bases((uint32_t)(x >> 16) & 0xffffu);
  }
  const uint64_t done = 8 * n8, tail = n - done;              // at most 7 bases
  if ((uint64_t)lane < tail) dst[done + lane] = base_at(seq, j0 + done + lane);
}

struct Timer {
  hipEvent_t a = nullptr, b = nullptr; hipStream_t st;
  explicit Timer(hipStream_t s) : st(s) { (void)hipEventCreate(&a); (void)hipEventCreate(&b); (void)hipEventRecord(a, st); }
  double stop() { float ms = 0; (void)hipEventRecord(b, st); (void)hipEventSynchronize(b); (void)hipEventElapsedTime(&ms, a, b); return ms; }
  ~Timer() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); }
};
inline unsigned blocks_of(uint64_t lanes) { return (unsigned)((lanes + 255) / 256); }
inline unsigned wave_blocks(lra_ctx* ctx, uint64_t waves) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((waves + 3) / 4, (uint64_t)ctx->num_cu * 32)); }
// an object's own arrays: an eighth of slack so that windows of about one size do not allocate anew; contents are not kept
template <typename T> struct Buf {
  T* p = nullptr; size_t n = 0;
  bool ensure(size_t want) {
    if (want <= n) return true;
    if (p) (void)hipFree(p);
    p = nullptr; n = 0;
    const size_t m = want + want / 8 + 16;
    if (hipMalloc((void**)&p, m * sizeof(T)) != hipSuccess) return false;
    n = m;
    return true;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};
inline double wall_ms(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

}  // namespace

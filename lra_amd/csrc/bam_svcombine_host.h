// lra_amd/csrc/bam_svcombine_host.h -- the arithmetic lra_sv_combine's kernels (bam_svcombine.hip) share with the host: the fraction as the object takes it,
// the partner test of Homcalls / Hetcalls (bedtools intersect -f F -r), the tiles of a table's reference range and the search of a row's partner through
// them.  Compiles alone: tools/micro/bam_svcombine_host_check.cpp runs it under the host sanitizers, the integer test against the single-precision one and
// the tile skip against all pairs.
#pragma once
#include <stdint.h>
#include <vector>

#if defined(__HIPCC__)
#define SVC_HD __host__ __device__ __forceinline__
#else
#define SVC_HD inline
#endif

constexpr int LRA_SVC_TILE = 256;

// frac_num / frac_den as given -> the fraction used.  0 / 0: 3 / 10 (the snakefile's -f 0.3).  false: den == 0, num == 0 or num > den.
inline bool lra_svc_frac(uint32_t num, uint32_t den, uint32_t* n, uint32_t* d) {
  if (!num && !den) { *n = 3; *d = 10; return true; }
  if (!den || !num || num > den) return false;
  *n = num; *d = den;
  return true;
}

// Rows a and b of one kind and one reference are partners when they share ov > 0 bases and ov is at least num / den of each: den ov >= num len for both.
// Rows are half-open with END > START, END < 2^32 (a BAM reference is below 2^31 bases, an insertion below 2^32), num and den 32 bits: the products fit
// unsigned 64-bit words.
// The float form.  bedtools tests (float)ov / (float)len >= 0.3f.  For len <= LRA_SVC_FLOAT_LEN = 2^24 both operands are exact floats and the quotient is
// the correctly rounded ov / len.  0.3f = 10066330 * 2^-25 lies above 3 / 10, its lower neighbour's midpoint 10066329.5 * 2^-25 lies 0.1 * 2^-25 below
// 3 / 10.  ov / len == 3 / 10 rounds to 0.3f: holds, as 10 ov >= 3 len does.  ov / len > 3 / 10 rounds to at least 0.3f: holds.  ov / len < 3 / 10 is below
// by at least 1 / (10 len) > 0.1 * 2^-25 for len < 2^25: it rounds below 0.3f and fails, as the integers do.  For 1 / 10: 0.1f = 13421773 * 2^-27, the
// midpoint lies 0.3 * 2^-27 below 1 / 10, and 1 / (10 len) exceeds that for len < 2^27 / 3.  So for len <= 2^24 the two forms agree for both fractions.
constexpr int64_t LRA_SVC_FLOAT_LEN = 1ll << 24;
SVC_HD bool lra_svc_partner(int64_t a_start, int64_t a_end, int64_t b_start, int64_t b_end, uint32_t num, uint32_t den) {
  const int64_t ov = (a_end < b_end ? a_end : b_end) - (a_start > b_start ? a_start : b_start);
  if (ov <= 0) return false;
  const uint64_t x = (uint64_t)den * (uint64_t)ov;
  return x >= (uint64_t)num * (uint64_t)(a_end - a_start) && x >= (uint64_t)num * (uint64_t)(b_end - b_start);
}

// Table B's rows [lo, hi) -- one reference's, in NR order -- in tiles of LRA_SVC_TILE rows from lo on; tile t's interval [t_lo[t], t_hi[t]) holds its rows'
// lowest START and highest END.  Does row [s, e) have a partner among them?  A tile whose interval shares no base with the row is passed over (ov > 0
// needs one).  There is no early exit on START: B is in NR order, and a long record's late variant precedes the next record's early one.
// Row: anything with .start and .end.
template <typename Row> SVC_HD bool lra_svc_has_partner(int64_t s, int64_t e, const Row* b, uint64_t lo, uint64_t hi, const int64_t* t_lo, const int64_t* t_hi,
                                                        uint32_t num, uint32_t den) {
  for (uint64_t t = 0; lo + t * LRA_SVC_TILE < hi; t++) {
    if (t_lo[t] >= e || t_hi[t] <= s) continue;
    const uint64_t k0 = lo + t * LRA_SVC_TILE, k1 = k0 + LRA_SVC_TILE < hi ? k0 + LRA_SVC_TILE : hi;
    for (uint64_t k = k0; k < k1; k++) if (lra_svc_partner(s, e, b[k].start, b[k].end, num, den)) return true;
  }
  return false;
}
// the tiles of rows [lo, hi) on the host, as svc_tiles computes them (for the check program and as the statement of what the kernel does)
template <typename Row> inline void lra_svc_tiles(const Row* b, uint64_t lo, uint64_t hi, std::vector<int64_t>* t_lo, std::vector<int64_t>* t_hi) {
  t_lo->clear(); t_hi->clear();
  for (uint64_t k0 = lo; k0 < hi; k0 += LRA_SVC_TILE) {
    int64_t a = INT64_MAX, z = INT64_MIN;
    for (uint64_t k = k0; k < hi && k < k0 + LRA_SVC_TILE; k++) { a = b[k].start < a ? b[k].start : a; z = b[k].end > z ? b[k].end : z; }
    t_lo->push_back(a); t_hi->push_back(z);
  }
}
// the first row of b[0, n), sorted by .ref, whose reference is at least r
template <typename Row> SVC_HD uint64_t lra_svc_ref_begin(const Row* b, uint64_t n, int32_t r) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (b[mid].ref >= r) hi = mid; else lo = mid + 1; }
  return lo;
}

// lra_amd/csrc/bam_svcalls_host.h -- the host bookkeeping of lra_bam_svcalls (bam_svcalls.hip) that needs no device, and the arithmetic its kernels share with
// the host: the options as the pass takes them, the mask as the kernels search it, the mask test, the merge's relation and one row's decision in a round, the ID
// stems, which passes are whole, and the bytes of a piece.  Compiles alone: tools/micro/bam_svcalls_host_check.cpp runs it under the host sanitizers, the
// rounds against the serial walk of the reference's mergeSV.py.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define SV_HD __host__ __device__ __forceinline__
#else
#define SV_HD inline
#endif

// min_size 0: 1 (a row needs a length: END > START is what the mask's merged form and the relation rely on)
inline uint32_t lra_sv_min_size(uint32_t min_size) { return min_size ? min_size : 1u; }

// ---- the mask ------------------------------------------------------------------------------------------------------------------------------------------------
// bedtools intersect -v: a row [start, end) is dropped when start < m.end && m.beg < end for an interval m of its reference.  The intervals of a reference,
// sorted by beg, with every interval that begins at or in front of the running end joined to it, are disjoint and apart (beg[k + 1] > end[k]); for a row
// with end > start the joined form drops exactly the rows the given intervals drop: a row that meets the union [b1, max(e1, e2)) of two intervals with
// b2 <= e1 but neither of them would have start >= e1 >= b2 >= end.  off[n_ref + 1] indexes beg / end by reference.
struct lra_sv_mask { std::vector<uint64_t> off; std::vector<int64_t> beg, end; };
inline bool lra_sv_mask_build(int n_ref, uint64_t n, const int32_t* ref_id, const int64_t* beg, const int64_t* end, lra_sv_mask* out, std::string* why) {
  std::vector<std::vector<std::pair<int64_t, int64_t>>> by((size_t)std::max(n_ref, 0));
  for (uint64_t k = 0; k < n; k++) {
    if (ref_id[k] < 0 || ref_id[k] >= n_ref) { *why = "interval " + std::to_string(k) + " names reference " + std::to_string(ref_id[k]) + " outside [0, " + std::to_string(n_ref) + ")"; return false; }
    if (beg[k] < 0 || end[k] < beg[k]) { *why = "interval " + std::to_string(k) + " is [" + std::to_string(beg[k]) + ", " + std::to_string(end[k]) + ")"; return false; }
    by[(size_t)ref_id[k]].push_back({beg[k], end[k]});
  }
  out->off.assign(1, 0); out->beg.clear(); out->end.clear();
  for (auto& v : by) {
    std::sort(v.begin(), v.end());
    const size_t first = out->beg.size();
    for (const auto& iv : v) {
      if (out->beg.size() > first && iv.first <= out->end.back()) out->end.back() = std::max(out->end.back(), iv.second);
      else { out->beg.push_back(iv.first); out->end.push_back(iv.second); }
    }
    out->off.push_back(out->beg.size());
  }
  return true;
}
// the joined intervals [lo, hi) of the row's reference: the first whose end lies behind start is the only one that can meet the row
SV_HD bool lra_sv_masked(const int64_t* beg, const int64_t* end, uint64_t lo, uint64_t hi, int64_t start, int64_t stop) {
  const uint64_t top = hi;
  while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (end[mid] > start) hi = mid; else lo = mid + 1; }
  return lo < top && beg[lo] < stop;                           // (the intervals behind it begin behind its end: further still)
}

// ---- the merge -------------------------------------------------------------------------------------------------------------------------------------------------
// mergeCalls' awk over bedtools intersect -wao of the table with itself, for the first row a and the second row b: $23 / ($3 - $2) >= 0.1 && $23 / ($14 - $13)
// > 0.1 with $23 = ov = min(END) - max(START) when that is positive (no shared base: 0, and 0 > 0.1 fails).  In integers: 10 ov >= len_a && 10 ov > len_b.
// awk divides in doubles; ov / len is the correctly rounded quotient and 0.1 the correctly rounded 1 / 10, so they are equal when 10 ov == len, and a
// quotient that is not 1 / 10 differs from it by at least 1 / (10 len) -- for any len below 2^49 far more than the ulp of 0.1 -- so the comparison falls as
// the integers do.  The asymmetry (>= for the first row, > for the second) is the snakefile's.
SV_HD bool lra_sv_related(int64_t a_start, int64_t a_end, int64_t b_start, int64_t b_end) {
  const int64_t ov = (a_end < b_end ? a_end : b_end) - (a_start > b_start ? a_start : b_start);
  return ov > 0 && 10 * ov >= a_end - a_start && 10 * ov > b_end - b_start;
}
// mergeSV.py: in NR order a row is kept unless an earlier KEPT row is related to it (a kept row adds its partners to `seen`; a dropped row adds nothing).
// One row's decision in a round, from the states of its in-neighbours (the earlier rows k with R(k, i)) as the round before left them.
enum { LRA_SV_OPEN = 0, LRA_SV_KEPT = 1, LRA_SV_DROPPED = 2 };
SV_HD uint32_t lra_sv_decide(const uint32_t* state, const uint32_t* in, uint64_t lo, uint64_t hi) {
  bool open = false;
  for (uint64_t e = lo; e < hi; e++) {
    const uint32_t s = state[in[e]];
    if (s == LRA_SV_KEPT) return LRA_SV_DROPPED;
    open = open || s == LRA_SV_OPEN;
  }
  return open ? LRA_SV_OPEN : LRA_SV_KEPT;
}
// the serial walk, and the rounds on the host as the device runs them (both for the check program and the documentation of what the kernels do)
inline std::vector<uint32_t> lra_sv_merge_serial(const std::vector<int64_t>& start, const std::vector<int64_t>& end) {
  std::vector<uint32_t> st(start.size(), LRA_SV_OPEN);
  for (size_t i = 0; i < st.size(); i++) {
    st[i] = LRA_SV_KEPT;
    for (size_t k = 0; k < i && st[i] == LRA_SV_KEPT; k++)
      if (st[k] == LRA_SV_KEPT && lra_sv_related(start[k], end[k], start[i], end[i])) st[i] = LRA_SV_DROPPED;
  }
  return st;
}
inline std::vector<uint32_t> lra_sv_merge_rounds(const std::vector<int64_t>& start, const std::vector<int64_t>& end, uint64_t* rounds) {
  const size_t m = start.size();
  std::vector<uint64_t> off(m + 1, 0); std::vector<uint32_t> in;
  for (size_t i = 0; i < m; i++) {
    for (size_t k = 0; k < i; k++) if (lra_sv_related(start[k], end[k], start[i], end[i])) in.push_back((uint32_t)k);
    off[i + 1] = in.size();
  }
  std::vector<uint32_t> a(m, LRA_SV_OPEN), b(m);
  *rounds = 0;
  for (;;) {
    bool any = false;
    for (size_t i = 0; i < m; i++) {
      b[i] = a[i] != LRA_SV_OPEN ? a[i] : lra_sv_decide(a.data(), in.data(), off[i], off[i + 1]);
      any = any || b[i] != a[i];
    }
    a.swap(b);
    if (!any) return a;
    ++*rounds;
  }
}

// ---- the pass -------------------------------------------------------------------------------------------------------------------------------------------------
// the merge and the numbering need every row of a reference: a region pass covers [0, the reference's length)
inline bool lra_sv_whole_reference(int64_t beg, int64_t end, uint64_t ref_len) { return beg == 0 && end >= 0 && (uint64_t)end >= ref_len; }
// <aligner>.<DEL|INS>.<hap>. in front of NR; NULL strings are the snakefile's words (its awk gets -v aln=aligner: the literal word)
inline std::string lra_sv_id_stem(const char* aligner, const char* hap, int del) {
  return std::string(aligner ? aligner : "aligner") + (del ? ".DEL." : ".INS.") + (hap ? hap : "maternal") + ".";
}
inline bool lra_sv_name_ok(const char* s) { for (; s && *s; s++) if ((unsigned char)*s < 0x21 || (unsigned char)*s > 0x7e) return false; return true; }

// The bytes of a piece, as bam_vcf_host.h's: false when a size does not fit size_t or the sum wraps.
constexpr uint64_t LRA_SV_VALUE_BYTES = 64, LRA_SV_TEXT_PAD = 64;
inline bool lra_sv_piece_bytes(uint64_t n_rows, uint64_t text_len, int want_text, int want_values, uint64_t* dev_text, uint64_t* host_text, uint64_t* value_bytes) {
  *dev_text = *host_text = *value_bytes = 0;
  if (want_text) {
    if (text_len > UINT64_MAX - LRA_SV_TEXT_PAD) return false;
    *dev_text = text_len + LRA_SV_TEXT_PAD; *host_text = text_len + 1;
  }
  if (n_rows > UINT64_MAX / LRA_SV_VALUE_BYTES) return false;
  *value_bytes = want_values ? n_rows * LRA_SV_VALUE_BYTES : 0;
  return *dev_text <= SIZE_MAX && *value_bytes <= SIZE_MAX;
}

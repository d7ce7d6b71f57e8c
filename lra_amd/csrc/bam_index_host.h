// lra_amd/csrc/bam_index_host.h -- the .bai file (SAM specification 5.2) of a coordinate-sorted BAM record stream: the arrays an index is written from,
// the writer of its bytes, and the serial walk of a raw stream that fills the arrays (lra_bam_index_host).  Plain C++, no HIP: bam_sort.hip fills the same
// arrays on the device and writes through the same writer; a stand-alone program can include this file alone.  The rules are in include/lra_hip.h.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include <algorithm>

constexpr uint64_t LRA_BAI_MEMBER = 65280;                    // LRA_BGZF_IN_MAX: the stream stage cuts a member every so many bytes
constexpr uint64_t LRA_BAI_MAX_REF = 1ull << 29;              // the longest reference the bins address
constexpr uint32_t LRA_BAI_PSEUDO_BIN = 37450;
constexpr uint64_t LRA_BAI_NONE = ~0ull;                      // a window no record touches

struct lra_bai_run { uint32_t ref, bin; uint64_t vbeg, vend; };
struct lra_bai_ref { uint64_t first = LRA_BAI_NONE, last = 0, n_mapped = 0, n_unmapped = 0, n_intv = 0; };   // (the counters of a reference, as the device keeps them)
struct lra_bai_arrays {
  std::vector<lra_bai_run> runs;                              // sorted by (ref, bin), file order within
  std::vector<lra_bai_ref> ref;
  std::vector<uint64_t> lin_off;                              // [n_ref + 1]: a reference's windows in lin
  std::vector<uint64_t> lin;                                  // filled backward: window w < n_intv holds its value
  uint64_t n_no_coor = 0;
};

inline uint64_t lra_bai_windows(uint64_t ref_len) { return ((ref_len + 16383) >> 14) + 1; }

// the virtual offset of byte u of the stream; member_off has n_members + 1 entries
inline uint64_t lra_bai_voff(uint64_t u, const uint64_t* member_off, uint64_t first) { return ((first + member_off[u / LRA_BAI_MEMBER]) << 16) | (u % LRA_BAI_MEMBER); }

inline void lra_bai_put32(std::vector<uint8_t>& o, uint32_t v) { for (int k = 0; k < 4; k++) o.push_back((uint8_t)(v >> (8 * k))); }
inline void lra_bai_put64(std::vector<uint8_t>& o, uint64_t v) { for (int k = 0; k < 8; k++) o.push_back((uint8_t)(v >> (8 * k))); }

inline void lra_bai_write(const lra_bai_arrays& A, std::vector<uint8_t>& o) {
  o.clear();
  o.push_back('B'); o.push_back('A'); o.push_back('I'); o.push_back(1);
  const size_t n_ref = A.ref.size();
  lra_bai_put32(o, (uint32_t)n_ref);
  size_t r = 0;
  for (size_t ref = 0; ref < n_ref; ref++) {
    size_t e = r;
    uint32_t n_bin = 0;
    while (e < A.runs.size() && A.runs[e].ref == ref) { if (e == r || A.runs[e].bin != A.runs[e - 1].bin) n_bin++; e++; }
    const lra_bai_ref& R = A.ref[ref];
    const bool has = e > r;
    lra_bai_put32(o, n_bin + (has ? 1 : 0));
    while (r < e) {
      size_t b = r;
      while (b < e && A.runs[b].bin == A.runs[r].bin) b++;
      lra_bai_put32(o, A.runs[r].bin);
      lra_bai_put32(o, (uint32_t)(b - r));
      for (; r < b; r++) { lra_bai_put64(o, A.runs[r].vbeg); lra_bai_put64(o, A.runs[r].vend); }
    }
    if (has) {
      lra_bai_put32(o, LRA_BAI_PSEUDO_BIN); lra_bai_put32(o, 2);
      lra_bai_put64(o, R.first); lra_bai_put64(o, R.last); lra_bai_put64(o, R.n_mapped); lra_bai_put64(o, R.n_unmapped);
    }
    lra_bai_put32(o, (uint32_t)R.n_intv);
    for (uint64_t w = 0; w < R.n_intv; w++) lra_bai_put64(o, A.lin[A.lin_off[ref] + w]);
  }
  lra_bai_put64(o, A.n_no_coor);
}

inline uint32_t lra_bai_le32(const uint8_t* p) { return p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// the arrays of the sorted raw stream; 0, or -1 for a stream that is not records back to back / a refID outside [-1, n_ref) / a reference too long
inline int lra_bai_walk(const uint8_t* s, uint64_t len, int n_ref, const uint64_t* ref_len, const uint64_t* member_off, uint64_t n_members, uint64_t first,
                        lra_bai_arrays& A) {
  if (n_ref < 0 || (len + LRA_BAI_MEMBER - 1) / LRA_BAI_MEMBER != n_members) return -1;
  A = lra_bai_arrays();
  A.ref.resize((size_t)n_ref);
  A.lin_off.assign((size_t)n_ref + 1, 0);
  for (int r = 0; r < n_ref; r++) {
    if (ref_len[r] > LRA_BAI_MAX_REF) return -1;
    A.lin_off[(size_t)r + 1] = A.lin_off[r] + lra_bai_windows(ref_len[r]);
  }
  A.lin.assign((size_t)A.lin_off[n_ref], LRA_BAI_NONE);
  std::vector<lra_bai_run> runs;
  for (uint64_t at = 0; at < len;) {
    if (len - at < 36) return -1;
    const uint64_t bs = lra_bai_le32(s + at);
    if (bs < 32 || bs > len - at - 4) return -1;
    const uint8_t* c = s + at + 4;
    const int32_t ref = (int32_t)lra_bai_le32(c), pos = (int32_t)lra_bai_le32(c + 4);
    const uint32_t l_name = c[8], bin = c[10] | ((uint32_t)c[11] << 8), n_cig = c[12] | ((uint32_t)c[13] << 8), flag = c[14] | ((uint32_t)c[15] << 8);
    if (32 + (uint64_t)l_name + 4ull * n_cig > bs || ref < -1 || ref >= n_ref) return -1;
    const uint64_t next = at + 4 + bs;
    if (ref < 0) { A.n_no_coor++; at = next; continue; }
    uint64_t span = 0;
    for (uint32_t k = 0; k < n_cig; k++) {
      const uint32_t op = lra_bai_le32(c + 32 + l_name + 4 * (uint64_t)k);
      if ((0x18du >> (op & 15)) & 1) span += op >> 4;            // M D N = X
    }
    const uint64_t vb = lra_bai_voff(at, member_off, first), ve = lra_bai_voff(next, member_off, first);
    if (runs.empty() || runs.back().ref != (uint32_t)ref || runs.back().bin != bin) runs.push_back(lra_bai_run{(uint32_t)ref, bin, vb, ve});
    else runs.back().vend = ve;
    lra_bai_ref& R = A.ref[ref];
    R.first = std::min(R.first, vb); R.last = std::max(R.last, ve);
    if (flag & 4) R.n_unmapped++; else R.n_mapped++;
    const uint64_t p0 = pos < 0 ? 0 : (uint64_t)pos, n_win = A.lin_off[(size_t)ref + 1] - A.lin_off[ref];
    const uint64_t w0 = std::min(p0 >> 14, n_win - 1), w1 = std::min((p0 + std::max<uint64_t>(span, 1) - 1) >> 14, n_win - 1);
    for (uint64_t w = w0; w <= w1; w++) { uint64_t& x = A.lin[A.lin_off[ref] + w]; x = std::min(x, vb); }
    R.n_intv = std::max(R.n_intv, w1 + 1);
    at = next;
  }
  std::stable_sort(runs.begin(), runs.end(), [](const lra_bai_run& a, const lra_bai_run& b) { return a.ref != b.ref ? a.ref < b.ref : a.bin < b.bin; });
  A.runs.swap(runs);
  for (int r = 0; r < n_ref; r++) {                            // the backward fill
    uint64_t carry = LRA_BAI_NONE;
    for (uint64_t w = A.ref[r].n_intv; w-- > 0;) { uint64_t& x = A.lin[A.lin_off[r] + w]; if (x == LRA_BAI_NONE) x = carry; else carry = x; }
  }
  return 0;
}

// lra_bam_index_host's body (two-call convention; the codes are LRA_OK 0 and LRA_ERR_INVALID -1)
inline int lra_bai_index(const uint8_t* stream, uint64_t len, int n_ref, const uint64_t* ref_len, const uint64_t* member_off, uint64_t n_members, uint64_t first,
                         uint8_t* out, uint64_t cap, uint64_t* out_len) {
  if (!out_len || n_ref < 0 || (len && !stream) || (n_ref && !ref_len) || !member_off) return -1;
  lra_bai_arrays A;
  if (lra_bai_walk(stream, len, n_ref, ref_len, member_off, n_members, first, A)) return -1;
  std::vector<uint8_t> o;
  lra_bai_write(A, o);
  *out_len = o.size();
  if (!out) return 0;
  if (cap < o.size()) return -1;
  memcpy(out, o.data(), o.size());
  return 0;
}

// lra_amd/csrc/bam_merge_host.h -- the host parts of lra_bam_merger (bam_merge.hip) that touch bytes and offsets: the reference table of a BAM header, the
// coalescing of a round's chunks with those of the rounds before, and the conversion of what the rounds left in stream offsets u -- chunks, per-reference
// first / last and counters, the linear index's minima -- into the arrays lra_bai_write takes.  Plain C++, no HIP: a stand-alone program can include this
// file alone (tools/micro/bam_merge_host_check.cpp runs it under the host sanitizers against lra_bam_index_host's serial walk).
#pragma once
#include "bam_index_host.h"
#include <string>

struct lra_merge_refs { int32_t n_ref = 0; std::vector<std::string> name; std::vector<uint64_t> len; };

// the reference table of the uncompressed header h[0, n): magic, l_text, text, n_ref, per reference l_name, name, l_ref; false: not a whole header
inline bool lra_merge_parse_refs(const uint8_t* h, size_t n, lra_merge_refs& T) {
  if (n < 12 || memcmp(h, "BAM\1", 4) != 0) return false;
  uint64_t at = 8 + (uint64_t)lra_bai_le32(h + 4);
  if (at + 4 > n) return false;
  T.n_ref = (int32_t)lra_bai_le32(h + at); at += 4;
  if (T.n_ref < 0) return false;
  for (int32_t i = 0; i < T.n_ref; i++) {
    if (at + 4 > n) return false;
    const uint64_t ln = lra_bai_le32(h + at);
    if (at + 8 + ln > n) return false;
    T.name.emplace_back((const char*)h + at + 4, ln ? ln - 1 : 0);
    T.len.push_back(lra_bai_le32(h + at + 4 + ln));
    at += 8 + ln;
  }
  return true;
}

struct lra_merge_chunk { uint64_t key, ubeg, uend; };         // key = ref << 16 | bin; [ubeg, uend) in stream offsets

// A round's n chunks behind those of the rounds before.  open_end != LRA_BAI_NONE: the round began inside the last chunk, which goes on to open_end.
inline void lra_merge_add_round(std::vector<lra_merge_chunk>& C, uint64_t open_end, const uint64_t* key, const uint64_t* beg, const uint64_t* end, uint64_t n) {
  if (open_end != LRA_BAI_NONE && !C.empty()) C.back().uend = open_end;
  for (uint64_t i = 0; i < n; i++) C.push_back(lra_merge_chunk{key[i], beg[i], end[i]});
}

// The writer's arrays.  C: the chunks in file order (a reference's are contiguous); order: C's indices with each reference's chunks stable by bin;
// stat[5 n_ref + 1]: per reference first u, last u, n_mapped, n_unmapped, n_intv, behind them n_no_coor; lin: per window the smallest start u of a record
// that touches it (LRA_BAI_NONE: none), lin_off[n_ref + 1]; moff: the complete member table.  voff is monotone in u, so minima, first and last convert.
inline void lra_merge_index_arrays(const std::vector<lra_merge_chunk>& C, const std::vector<uint32_t>& order, const unsigned long long* stat, std::vector<uint64_t> lin,
                                   const std::vector<uint64_t>& lin_off, const uint64_t* moff, uint64_t first, lra_bai_arrays& A) {
  const size_t n_ref = lin_off.size() - 1;
  A = lra_bai_arrays();
  A.ref.resize(n_ref);
  A.lin_off = lin_off;
  A.runs.reserve(C.size());
  for (size_t i = 0; i < C.size(); i++) {
    const lra_merge_chunk& c = C[order[i]];
    A.runs.push_back(lra_bai_run{(uint32_t)(c.key >> 16), (uint32_t)(c.key & 0xffffu), lra_bai_voff(c.ubeg, moff, first), lra_bai_voff(c.uend, moff, first)});
  }
  for (size_t r = 0; r < n_ref; r++) {
    lra_bai_ref& R = A.ref[r];
    const unsigned long long* s = stat + 5 * r;
    R.first = s[0] == LRA_BAI_NONE ? LRA_BAI_NONE : lra_bai_voff(s[0], moff, first);
    R.last = (s[2] + s[3]) ? lra_bai_voff(s[1], moff, first) : 0;
    R.n_mapped = s[2]; R.n_unmapped = s[3]; R.n_intv = s[4];
    uint64_t carry = LRA_BAI_NONE;                             // the backward fill, with the conversion
    for (uint64_t w = R.n_intv; w-- > 0;) {
      uint64_t& x = lin[lin_off[r] + w];
      if (x == LRA_BAI_NONE) x = carry; else { x = lra_bai_voff(x, moff, first); carry = x; }
    }
  }
  A.lin.swap(lin);
  A.n_no_coor = stat[5 * n_ref];
}

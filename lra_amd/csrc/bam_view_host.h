// lra_amd/csrc/bam_view_host.h -- the host parts of lra_bam_view (bam_view.hip) that touch the bytes of a .bai file (SAM specification 5.2): the reader of
// an index and the planner that turns a region into the chunks of the file to read.  Plain C++, no HIP: a stand-alone program can include this file alone
// (tools/micro/bam_view_host_check.cpp runs it under the host sanitizers over whole and truncated indexes).  lra_bai_query_host is reader + planner.
//
// The reader checks every count and length against the bytes that remain before it uses it; the pseudo-bin 37450 is recognised (its two "chunks" are
// the reference's first / last offsets and its counters) and is not a bin.  The trailing n_no_coor is optional, as the specification has it.
// The planner (tests/bai_text.py's Reader.query, written out): the chunks of reg2bins(beg, end)'s bins; min_off = lin[beg >> 14] -- a window behind the last
// one means no record reaches beg or starts behind it: the plan is empty --; every chunk's start raised to min_off, a chunk that this empties dropped; the
// chunks sorted by start and those that overlap or touch merged.  The plan is ascending and disjoint: no record is read twice.
#pragma once
#include "bam_index_host.h"
#include <string>

struct lra_bai_chunk { uint64_t beg, end; };                  // virtual offsets, [beg, end)
struct lra_bai_bin { uint32_t bin; uint64_t c0, c1; };        // the bin's chunks are chunk[c0, c1)
struct lra_bai_ref_index {
  std::vector<lra_bai_bin> bins;                              // in file order, the pseudo-bin left out
  std::vector<lra_bai_chunk> chunk;
  std::vector<uint64_t> lin;
  bool has_meta = false; uint64_t first = 0, last = 0, n_mapped = 0, n_unmapped = 0;
};
struct lra_bai_file { std::vector<lra_bai_ref_index> ref; bool has_no_coor = false; uint64_t n_no_coor = 0; };

inline uint64_t lra_bai_le64(const uint8_t* p) { return (uint64_t)lra_bai_le32(p) | ((uint64_t)lra_bai_le32(p + 4) << 32); }

// The index in b[0, n).  expect_n_ref >= 0: the reference count of the BAM header it must have.  false: *why names the field.
inline bool lra_bai_read(const uint8_t* b, uint64_t n, int expect_n_ref, lra_bai_file& X, std::string& why) {
  X = lra_bai_file();
  uint64_t at = 0;
  auto left = [&]() { return n - at; };
  auto bad = [&](const std::string& s) { why = s + " (at byte " + std::to_string(at) + " of the index)"; return false; };
  if (left() < 8) return bad("the index is shorter than its magic and n_ref");
  if (memcmp(b, "BAI\1", 4) != 0) return bad("not a .bai index (no BAI\\1 magic)");
  const int32_t n_ref = (int32_t)lra_bai_le32(b + 4);
  at = 8;
  if (n_ref < 0) return bad("a negative n_ref");
  if (expect_n_ref >= 0 && n_ref != expect_n_ref)
    return bad("the index has " + std::to_string(n_ref) + " references, the BAM header has " + std::to_string(expect_n_ref));
  if ((uint64_t)n_ref > left() / 8) return bad("n_ref is more than the index can hold");   // (a reference takes at least n_bin and n_intv)
  X.ref.resize((size_t)n_ref);
  for (int32_t r = 0; r < n_ref; r++) {
    lra_bai_ref_index& R = X.ref[(size_t)r];
    const std::string who = "reference " + std::to_string(r) + ": ";
    if (left() < 4) return bad(who + "the index ends in front of n_bin");
    const int32_t n_bin = (int32_t)lra_bai_le32(b + at);
    if (n_bin < 0) return bad(who + "a negative n_bin");
    at += 4;
    if ((uint64_t)n_bin > left() / 8) return bad(who + "n_bin is more than the index can hold");
    for (int32_t k = 0; k < n_bin; k++) {
      if (left() < 8) return bad(who + "the index ends inside a bin's header");
      const uint32_t bin = lra_bai_le32(b + at);
      const int32_t n_chunk = (int32_t)lra_bai_le32(b + at + 4);
      if (n_chunk < 0) { at += 4; return bad(who + "a negative n_chunk"); }
      at += 8;
      if ((uint64_t)n_chunk > left() / 16) return bad(who + "n_chunk is more than the index can hold");
      if (bin == LRA_BAI_PSEUDO_BIN) {
        if (n_chunk != 2) return bad(who + "the pseudo-bin 37450 does not have two chunks");
        R.has_meta = true;
        R.first = lra_bai_le64(b + at); R.last = lra_bai_le64(b + at + 8); R.n_mapped = lra_bai_le64(b + at + 16); R.n_unmapped = lra_bai_le64(b + at + 24);
        at += 32;
        continue;
      }
      if (bin > LRA_BAI_PSEUDO_BIN) return bad(who + "bin " + std::to_string(bin) + " is not a bin of the index");
      lra_bai_bin B{bin, R.chunk.size(), 0};
      for (int32_t c = 0; c < n_chunk; c++, at += 16) {
        const lra_bai_chunk ch{lra_bai_le64(b + at), lra_bai_le64(b + at + 8)};
        if (ch.end < ch.beg) return bad(who + "a chunk of bin " + std::to_string(bin) + " ends in front of its start");
        R.chunk.push_back(ch);
      }
      B.c1 = R.chunk.size();
      R.bins.push_back(B);
    }
    if (left() < 4) return bad(who + "the index ends in front of n_intv");
    const int32_t n_intv = (int32_t)lra_bai_le32(b + at);
    if (n_intv < 0) return bad(who + "a negative n_intv");
    at += 4;
    if ((uint64_t)n_intv > left() / 8) return bad(who + "n_intv is more than the index can hold");
    R.lin.resize((size_t)n_intv);
    for (int32_t w = 0; w < n_intv; w++, at += 8) R.lin[(size_t)w] = lra_bai_le64(b + at);
  }
  if (left() == 0) return true;
  if (left() < 8) return bad("the index ends inside n_no_coor");
  X.has_no_coor = true; X.n_no_coor = lra_bai_le64(b + at);
  at += 8;
  if (left()) return bad("bytes behind n_no_coor");
  return true;
}

// the bins that may hold a record overlapping [beg, end), end > beg (SAM specification 5.3), appended to out
inline void lra_bai_reg2bins(uint64_t beg, uint64_t end, std::vector<uint32_t>& out) {
  end -= 1;
  out.push_back(0);
  const int sh[5] = {26, 23, 20, 17, 14};
  const uint32_t base[5] = {1, 9, 73, 585, 4681};
  for (int l = 0; l < 5; l++) for (uint64_t k = beg >> sh[l]; k <= end >> sh[l]; k++) out.push_back(base[l] + (uint32_t)k);
}

// The plan of [beg, end) on reference ref_id (0-based, half-open; end above 2^29 counts as 2^29).  false: ref_id outside the index, or beg > end.
// beg == end is a valid region that no record overlaps: the plan is empty.
inline bool lra_bai_plan(const lra_bai_file& X, int64_t ref_id, int64_t beg, int64_t end, std::vector<lra_bai_chunk>& plan, std::string& why) {
  plan.clear();
  if (ref_id < 0 || (uint64_t)ref_id >= X.ref.size()) { why = "reference " + std::to_string(ref_id) + " is outside [0, " + std::to_string(X.ref.size()) + ")"; return false; }
  if (beg < 0 || beg > end) { why = "the region [" + std::to_string(beg) + ", " + std::to_string(end) + ") is not a region"; return false; }
  const lra_bai_ref_index& R = X.ref[(size_t)ref_id];
  const uint64_t b = (uint64_t)beg, e = std::min<uint64_t>((uint64_t)end, LRA_BAI_MAX_REF);
  if (b >= e) return true;
  const uint64_t w = b >> 14;
  if (w >= R.lin.size()) return true;
  const uint64_t min_off = R.lin[(size_t)w];
  std::vector<uint32_t> want;
  lra_bai_reg2bins(b, e, want);
  std::sort(want.begin(), want.end());
  for (const lra_bai_bin& B : R.bins) {
    if (!std::binary_search(want.begin(), want.end(), B.bin)) continue;
    for (uint64_t c = B.c0; c < B.c1; c++) {
      const lra_bai_chunk ch{std::max(R.chunk[(size_t)c].beg, min_off), R.chunk[(size_t)c].end};
      if (ch.beg < ch.end) plan.push_back(ch);
    }
  }
  std::sort(plan.begin(), plan.end(), [](const lra_bai_chunk& x, const lra_bai_chunk& y) { return x.beg != y.beg ? x.beg < y.beg : x.end < y.end; });
  size_t o = 0;
  for (size_t i = 0; i < plan.size(); i++) {
    if (o && plan[i].beg <= plan[o - 1].end) plan[o - 1].end = std::max(plan[o - 1].end, plan[i].end);
    else plan[o++] = plan[i];
  }
  plan.resize(o);
  return true;
}

// lra_bai_query_host's body: 0, or -1 (LRA_ERR_INVALID) with *why
inline int lra_bai_query(const uint8_t* bai, uint64_t bai_len, int n_ref, int64_t ref_id, int64_t beg, int64_t end, std::vector<lra_bai_chunk>& plan, std::string& why) {
  lra_bai_file X;
  if (!bai && bai_len) { why = "no index bytes"; return -1; }
  if (!lra_bai_read(bai, bai_len, n_ref, X, why)) return -1;
  return lra_bai_plan(X, ref_id, beg, end, plan, why) ? 0 : -1;
}

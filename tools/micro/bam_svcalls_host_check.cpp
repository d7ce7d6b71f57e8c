// tools/micro/bam_svcalls_host_check.cpp -- the host bookkeeping of lra_bam_svcalls (lra_amd/csrc/bam_svcalls_host.h) under the host sanitizers, as a program of
// its own:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I lra_amd/csrc tools/micro/bam_svcalls_host_check.cpp -o /tmp/sv_check && /tmp/sv_check
// The joined mask, searched as the kernels search it, must drop exactly the rows the given intervals drop by bedtools' rule, inside heap arrays of exactly the
// intervals' size; the relation must be the double test of the snakefile's awk; the rounds must decide what the serial walk of mergeSV.py decides, for random
// tables, chains, cliques and rows numbered against their positions; the options, the ID stems, the whole-reference test and the piece sizes.
#include "bam_svcalls_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

int main() {
  std::mt19937_64 g(11);
  // the mask
  uint64_t n_rows = 0, n_masked = 0;
  for (int it = 0; it < 3000; it++) {
    const int n_ref = 1 + (int)(g() % 3);
    const uint64_t n = g() % 12;
    std::vector<int32_t> ref(n); std::vector<int64_t> beg(n), end(n);
    for (uint64_t k = 0; k < n; k++) { ref[k] = (int32_t)(g() % n_ref); beg[k] = (int64_t)(g() % 200); end[k] = beg[k] + (int64_t)(g() % 4 == 0 ? 0 : g() % 40); }
    lra_sv_mask m; std::string why;
    CHECK(lra_sv_mask_build(n_ref, n, ref.data(), beg.data(), end.data(), &m, &why));
    CHECK(m.off.size() == (size_t)n_ref + 1 && m.off.back() == m.beg.size() && m.beg.size() == m.end.size() && m.beg.size() <= n);
    // exact-size heap copies: a search that leaves its range is a sanitizer report
    int64_t* hb = (int64_t*)malloc(m.beg.size() * 8 + 1); int64_t* he = (int64_t*)malloc(m.end.size() * 8 + 1);
    if (!m.beg.empty()) { memcpy(hb, m.beg.data(), m.beg.size() * 8); memcpy(he, m.end.data(), m.end.size() * 8); }
    for (int r = 0; r < n_ref; r++)
      for (uint64_t k = m.off[r]; k + 1 < m.off[r + 1]; k++) CHECK(m.beg[k + 1] > m.end[k]);   // disjoint and apart
    for (int q = 0; q < 60; q++) {
      const int32_t r = (int32_t)(g() % n_ref);
      const int64_t s = (int64_t)(g() % 260), e = s + 1 + (int64_t)(g() % 30);
      bool want = false;
      for (uint64_t k = 0; k < n; k++) want = want || (ref[k] == r && s < end[k] && beg[k] < e);
      const bool got = lra_sv_masked(hb, he, m.off[r], m.off[r + 1], s, e);
      CHECK(got == want);
      n_rows++; n_masked += got;
    }
    free(hb); free(he);
  }
  CHECK(n_masked > n_rows / 10 && n_masked < n_rows);
  {
    lra_sv_mask m; std::string why;
    const int32_t r1[1] = {2}; const int64_t b1[1] = {5}, e1[1] = {9}, e2[1] = {4}, b3[1] = {-1};
    CHECK(!lra_sv_mask_build(2, 1, r1, b1, e1, &m, &why) && why.find("outside [0, 2)") != std::string::npos);
    const int32_t r0[1] = {0};
    CHECK(!lra_sv_mask_build(2, 1, r0, b1, e2, &m, &why) && !lra_sv_mask_build(2, 1, r0, b3, e1, &m, &why));
    CHECK(lra_sv_mask_build(2, 0, nullptr, nullptr, nullptr, &m, &why) && m.off.size() == 3 && m.beg.empty());
    CHECK(!lra_sv_masked(nullptr, nullptr, 0, 0, 5, 9));
    // touching is no overlap; one shared base is
    const int64_t tb[1] = {100}, te[1] = {140};
    CHECK(!lra_sv_masked(tb, te, 0, 1, 140, 180) && !lra_sv_masked(tb, te, 0, 1, 60, 100) && lra_sv_masked(tb, te, 0, 1, 139, 180) && lra_sv_masked(tb, te, 0, 1, 60, 101));
  }

  // the relation: the integers against awk's doubles
  for (int it = 0; it < 400000; it++) {
    const int64_t big = it % 3 == 0 ? (int64_t)(g() % 2000000000) : 0;
    const int64_t a0 = big + (int64_t)(g() % 300), a1 = a0 + 1 + (int64_t)(it % 5 == 0 ? g() % 3000000 : g() % 200);
    const int64_t b0 = big + (int64_t)(g() % 300), b1 = b0 + 1 + (int64_t)(it % 7 == 0 ? g() % 3000000 : g() % 200);
    const int64_t ov = std::max<int64_t>(0, std::min(a1, b1) - std::max(a0, b0));
    const bool want = (double)ov / (double)(a1 - a0) >= 0.1 && (double)ov / (double)(b1 - b0) > 0.1;
    CHECK(lra_sv_related(a0, a1, b0, b1) == want);
  }
  CHECK(lra_sv_related(0, 100, 90, 140) && !lra_sv_related(90, 140, 0, 100));                   // 10 ov == len: the first row's >=, the second row's >
  CHECK(!lra_sv_related(0, 50, 50, 100) && !lra_sv_related(50, 100, 0, 50) && !lra_sv_related(0, 10, 9, 19) && lra_sv_related(0, 10, 8, 18) && lra_sv_related(5, 6, 5, 6));

  // the rounds against the serial walk
  uint64_t most = 0, tables = 0;
  auto same = [&](const std::vector<int64_t>& s, const std::vector<int64_t>& e, uint64_t* rounds) {
    const std::vector<uint32_t> a = lra_sv_merge_serial(s, e), b = lra_sv_merge_rounds(s, e, rounds);
    CHECK(a == b);
    for (uint32_t x : b) CHECK(x == LRA_SV_KEPT || x == LRA_SV_DROPPED);
    most = std::max(most, *rounds); tables++;
    return b;
  };
  for (int it = 0; it < 4000; it++) {
    const size_t m = (size_t)(g() % 60);
    std::vector<int64_t> s(m), e(m);
    const int64_t room = 50 + (int64_t)(g() % 2000);
    for (size_t i = 0; i < m; i++) { s[i] = (int64_t)(g() % room); e[i] = s[i] + 1 + (int64_t)(g() % 120); }
    uint64_t r = 0;
    same(s, e, &r);
  }
  {
    uint64_t r = 0;
    std::vector<int64_t> s, e;
    for (int k = 0; k < 200; k++) { s.push_back(80 * k); e.push_back(80 * k + 100); }          // a chain: each row related to its successor only
    std::vector<uint32_t> st = same(s, e, &r);
    for (int k = 0; k < 200; k++) CHECK(st[k] == (k % 2 ? LRA_SV_DROPPED : LRA_SV_KEPT));
    CHECK(r == 200);
    s.clear(); e.clear();
    for (int k = 0; k < 257; k++) { s.push_back(k); e.push_back(5000 + k); }                    // mutually related: the first is kept
    st = same(s, e, &r);
    CHECK(st[0] == LRA_SV_KEPT && std::count(st.begin(), st.end(), (uint32_t)LRA_SV_KEPT) == 1 && r == 2);
    std::vector<int64_t> s3 = {0, 80, 160}, e3 = {100, 180, 260};                               // A ~ B ~ C: B goes, C stays
    st = same(s3, e3, &r);
    CHECK(st[0] == LRA_SV_KEPT && st[1] == LRA_SV_DROPPED && st[2] == LRA_SV_KEPT);
    std::vector<int64_t> s5 = {500, 100, 520, 110, 0}, e5 = {600, 200, 620, 210, 50};           // NR order against START order
    st = same(s5, e5, &r);
    CHECK(st[0] == LRA_SV_KEPT && st[1] == LRA_SV_KEPT && st[2] == LRA_SV_DROPPED && st[3] == LRA_SV_DROPPED && st[4] == LRA_SV_KEPT);
    CHECK(same({}, {}, &r).empty() && r == 0);
  }

  // the options, the stems, the pass, a piece's bytes
  CHECK(lra_sv_min_size(0) == 1 && lra_sv_min_size(40) == 40);
  CHECK(lra_sv_id_stem(nullptr, nullptr, 1) == "aligner.DEL.maternal." && lra_sv_id_stem("lra", "paternal", 0) == "lra.INS.paternal.");
  CHECK(lra_sv_name_ok("lra") && lra_sv_name_ok(nullptr) && lra_sv_name_ok("") && !lra_sv_name_ok("a b") && !lra_sv_name_ok("a\tb") && !lra_sv_name_ok("\xc3\xa4"));
  CHECK(lra_sv_whole_reference(0, 100, 100) && lra_sv_whole_reference(0, 1ll << 40, 100) && !lra_sv_whole_reference(1, 100, 100) && !lra_sv_whole_reference(0, 99, 100) &&
        !lra_sv_whole_reference(0, -1, 0) && lra_sv_whole_reference(0, 0, 0));
  uint64_t a, b, c;
  CHECK(lra_sv_piece_bytes(3, 1000, 1, 1, &a, &b, &c) && a == 1064 && b == 1001 && c == 192);
  CHECK(lra_sv_piece_bytes(3, 1000, 0, 1, &a, &b, &c) && a == 0 && b == 0 && c == 192 && lra_sv_piece_bytes(0, 0, 1, 1, &a, &b, &c) && a == 64 && b == 1 && c == 0);
  CHECK(!lra_sv_piece_bytes(1, UINT64_MAX - 10, 1, 0, &a, &b, &c) && !lra_sv_piece_bytes(UINT64_MAX / 8, 10, 1, 1, &a, &b, &c));

  if (fails) printf("bam_svcalls_host_check: %d checks FAILED\n", fails);
  else printf("bam_svcalls_host_check: clean (%llu rows against the mask, %llu tables merged, %llu rounds at most)\n", (unsigned long long)n_rows, (unsigned long long)tables,
              (unsigned long long)most);
  return fails ? 1 : 0;
}

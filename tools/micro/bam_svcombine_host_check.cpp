// tools/micro/bam_svcombine_host_check.cpp -- the arithmetic of lra_sv_combine (lra_amd/csrc/bam_svcombine_host.h) under the host sanitizers, as a program of
// its own:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I lra_amd/csrc tools/micro/bam_svcombine_host_check.cpp -o /tmp/svc_check && /tmp/svc_check
// The integer partner test must be the single-precision test bedtools makes, (float)ov / (float)len >= 0.3f (and 0.1f): for every ov <= len <= 4096, and for
// sampled len up to LRA_SVC_FLOAT_LEN with ov at and around the fraction's edge; the search through the tiles, inside heap arrays of exactly the tables'
// size, must find a partner exactly when the all-pairs form does, for random tables by reference in NR order, with ranges of 0, 255, 256, 257 and 513 rows;
// the fraction as the object takes it.
#include "bam_svcombine_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

struct Row { int64_t start, end; int32_t ref; };

// one row of length len against a row that shares ov bases with it and is no shorter: the integer form is then the test on this row alone
static bool int_form(int64_t ov, int64_t len, uint32_t num, uint32_t den) { return lra_svc_partner(0, len, len - ov, len - ov + len, num, den); }
static bool float_form(int64_t ov, int64_t len, float lit) { volatile float q = (float)ov / (float)len; return q >= lit; }

int main() {
  std::mt19937_64 g(29);
  // the fraction
  uint32_t n = 0, d = 0;
  CHECK(lra_svc_frac(0, 0, &n, &d) && n == 3 && d == 10);
  CHECK(lra_svc_frac(1, 10, &n, &d) && n == 1 && d == 10);
  CHECK(lra_svc_frac(7, 7, &n, &d) && n == 7 && d == 7);
  CHECK(!lra_svc_frac(0, 7, &n, &d) && !lra_svc_frac(4, 3, &n, &d) && !lra_svc_frac(1, 0, &n, &d));
  // the float form, exhaustively
  uint64_t n_tests = 0, n_edge = 0;
  const struct { uint32_t num, den; float lit; } FR[2] = {{3, 10, 0.3f}, {1, 10, 0.1f}};
  for (const auto& f : FR) {
    for (int64_t len = 1; len <= 4096; len++)
      for (int64_t ov = 1; ov <= len; ov++) { CHECK(int_form(ov, len, f.num, f.den) == float_form(ov, len, f.lit)); n_tests++; }
    // sampled up to the bound: around the edge ov = ceil(num len / den), where the forms could part, and anywhere
    for (int it = 0; it < 4000000; it++) {
      const int64_t len = it < 64 ? LRA_SVC_FLOAT_LEN - it : 1 + (int64_t)(g() % (uint64_t)LRA_SVC_FLOAT_LEN);
      const int64_t edge = (int64_t)(((uint64_t)f.num * (uint64_t)len + f.den - 1) / f.den);
      for (int64_t ov = edge - 2; ov <= edge + 2; ov++)
        if (ov >= 1 && ov <= len) { CHECK(int_form(ov, len, f.num, f.den) == float_form(ov, len, f.lit)); n_edge++; }
      const int64_t ov = 1 + (int64_t)(g() % (uint64_t)len);
      CHECK(int_form(ov, len, f.num, f.den) == float_form(ov, len, f.lit));
    }
  }
  // the test itself: both rows, symmetric, touching
  CHECK(lra_svc_partner(100, 110, 107, 117, 3, 10) && !lra_svc_partner(100, 110, 108, 118, 3, 10) && !lra_svc_partner(100, 110, 107, 118, 3, 10));
  CHECK(!lra_svc_partner(100, 110, 110, 120, 3, 10) && lra_svc_partner(100, 110, 90, 123, 3, 10) && !lra_svc_partner(100, 110, 90, 124, 3, 10));
  CHECK(lra_svc_partner(0, 4000000000ll, 0, 4000000000ll, 4000000000u, 4000000000u) && !lra_svc_partner(0, 4000000000ll, 1, 4000000001ll, 4000000000u, 4000000000u) &&
        lra_svc_partner(0, 4000000000ll, 1, 4000000001ll, 3999999999u, 4000000000u));   // 1.6e19: the products stay inside 64 unsigned bits
  // the tiles against all pairs
  uint64_t n_rows = 0, n_with = 0, n_skipped = 0;
  for (int it = 0; it < 400; it++) {
    const int n_ref = 1 + (int)(g() % 4);
    const uint32_t num = it % 3 ? 3 : 1, den = 10;
    static const uint64_t SIZES[8] = {0, 1, 255, 256, 257, 513, 40, 700};
    std::vector<Row> b;
    const int64_t spread = it % 2 ? 3000 : 200000;
    for (int r = 0; r < n_ref; r++) {
      const uint64_t m = SIZES[g() % 8];
      for (uint64_t k = 0; k < m; k++) {
        // NR order is nearly START order, with a long row now and then and a late variant in front of an early one
        const int64_t s = (int64_t)(k * (uint64_t)spread / (m + 1)) + (int64_t)(g() % 300), len = g() % 50 == 0 ? 1 + (int64_t)(g() % (uint64_t)spread) : 1 + (int64_t)(g() % 120);
        b.push_back(Row{s, s + len, r});
      }
    }
    Row* hb = (Row*)malloc(b.size() * sizeof(Row) + 1);                             // exact size: a search that leaves its range is a sanitizer report
    if (!b.empty()) memcpy(hb, b.data(), b.size() * sizeof(Row));
    for (int r = 0; r < n_ref; r++) {
      const uint64_t lo = lra_svc_ref_begin(hb, b.size(), r), hi = lra_svc_ref_begin(hb, b.size(), r + 1);
      uint64_t want_lo = 0, want_hi = 0;
      for (const Row& x : b) { want_lo += x.ref < r; want_hi += x.ref <= r; }
      CHECK(lo == want_lo && hi == want_hi);
      std::vector<int64_t> t_lo, t_hi;
      lra_svc_tiles(hb, lo, hi, &t_lo, &t_hi);
      CHECK(t_lo.size() == (hi - lo + LRA_SVC_TILE - 1) / LRA_SVC_TILE);
      int64_t* hl = (int64_t*)malloc(t_lo.size() * 8 + 1); int64_t* hh = (int64_t*)malloc(t_hi.size() * 8 + 1);
      if (!t_lo.empty()) { memcpy(hl, t_lo.data(), t_lo.size() * 8); memcpy(hh, t_hi.data(), t_hi.size() * 8); }
      for (int q = 0; q < 300; q++) {
        const int64_t s = (int64_t)(g() % (uint64_t)(spread + 400)), e = s + 1 + (int64_t)(g() % (q % 7 ? 150 : 5000));
        bool want = false;
        for (uint64_t k = lo; k < hi; k++) want = want || lra_svc_partner(s, e, hb[k].start, hb[k].end, num, den);
        CHECK(lra_svc_has_partner(s, e, hb, lo, hi, hl, hh, num, den) == want);
        for (size_t t = 0; t < t_lo.size(); t++) n_skipped += t_lo[t] >= e || t_hi[t] <= s;
        n_rows++; n_with += want;
      }
      free(hl); free(hh);
    }
    free(hb);
  }
  CHECK(n_with > n_rows / 50 && n_with < n_rows && n_skipped > 0);
  printf("bam_svcombine_host_check: %llu exhaustive and %llu edge comparisons of the float form up to len %lld; %llu rows against tiled tables, %llu with a partner, "
         "%llu tiles passed over: %s\n", (unsigned long long)n_tests, (unsigned long long)n_edge, (long long)LRA_SVC_FLOAT_LEN, (unsigned long long)n_rows,
         (unsigned long long)n_with, (unsigned long long)n_skipped, fails ? "FAILED" : "ok");
  return fails ? 1 : 0;
}

// tools/micro/bam_vcf_host_check.cpp -- the host bookkeeping of lra_bam_vcf (lra_amd/csrc/bam_vcf_host.h) under the host sanitizers, as a program of its own:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I lra_amd/csrc tools/micro/bam_vcf_host_check.cpp -o /tmp/vcf_check && /tmp/vcf_check
// A serial walk over random CIGARs (include/lra_hip.h's rules, with the counters the kernels hand to lra_vcf_shape_of) must index SEQ and the genome inside
// their heap blocks of exactly the bytes given -- ALT = SEQ[aq, aq + alt_len), REF = genome[r0 - 1, r0 - 1 + ref_len) -- for records the window would not
// refuse; the region test must keep exactly the anchors of [beg, end); the first refusal of a window must be the lowest record and, on one record, the
// lowest kind, whatever the order the checks report in; the piece sizes must refuse what wraps; the tables must name the first reference that differs.
#include "bam_vcf_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

struct Op { uint32_t len; int cls; };                         // 0 none, 1 match, 2 ins, 3 del

int main() {
  std::mt19937_64 g(7);
  // the walk: every variant's REF and ALT lie inside the record's SEQ and its reference
  uint64_t n_var = 0, n_kept = 0;
  for (int it = 0; it < 20000; it++) {
    const int n_op = 1 + (int)(g() % 12);
    std::vector<Op> ops;
    uint64_t l_seq = 0, span = 0;
    for (int k = 0; k < n_op; k++) {
      Op o; o.cls = (int)(g() % 4); o.len = (uint32_t)(g() % 5 == 0 ? 0 : g() % 40);
      if (!o.len) o.cls = 0;
      ops.push_back(o);
      if (o.cls == 1 || o.cls == 2) l_seq += o.len;
      if (o.cls == 1 || o.cls == 3) span += o.len;
    }
    const int64_t pos = (int64_t)(g() % 50);
    const uint64_t ref_len = (uint64_t)pos + span + g() % 3;
    unsigned char* seq = (unsigned char*)malloc(l_seq ? l_seq : 1);
    unsigned char* ref = (unsigned char*)malloc(ref_len ? ref_len : 1);
    memset(seq, 'A', l_seq); memset(ref, 'C', ref_len);
    const int64_t beg = (int64_t)(g() % (ref_len + 1)), end = beg + (int64_t)(g() % (ref_len + 1));
    uint64_t q = 0; int64_t r = pos, r0 = 0; bool have = false; uint64_t aq = 0; int run = 0;
    auto close = [&](uint64_t q1, int64_t r1) {
      const lra_vcf_shape s = lra_vcf_shape_of(run == 3, aq, r0, q1, r1);
      n_var++;
      CHECK(s.svlen == (int64_t)s.alt_len - (int64_t)s.ref_len && s.alt_len >= 1 && s.ref_len >= 1);
      CHECK(aq + s.alt_len <= l_seq && r0 - 1 >= 0 && (uint64_t)(r0 - 1) + s.ref_len <= ref_len);
      unsigned sum = 0;
      for (uint64_t k = 0; k < s.alt_len; k++) sum += seq[aq + k];
      for (uint64_t k = 0; k < s.ref_len; k++) sum += ref[(uint64_t)(r0 - 1) + k];
      CHECK(sum == 'A' * s.alt_len + 'C' * s.ref_len);
      const bool in = lra_vcf_anchor_in(1, r0 - 1, beg, end);
      CHECK(in == (r0 - 1 >= beg && r0 - 1 < end) && lra_vcf_anchor_in(0, r0 - 1, beg, end));
      CHECK(lra_vcf_long_enough(s.svlen, 1) == (s.svlen != 0));
      if (in && lra_vcf_long_enough(s.svlen, 3)) n_kept++;
    };
    for (const Op& o : ops) {
      if (!o.cls) continue;
      if (run && o.cls != run) { close(q, r); run = 0; }
      if (o.cls == 1) { q += o.len; r += o.len; aq = q - 1; have = true; continue; }
      if (have && !run) { run = o.cls; r0 = r; }
      if (o.cls == 2) q += o.len; else r += o.len;
    }
    free(seq); free(ref);
  }
  CHECK(n_var > 10000 && n_kept > 100);
  CHECK(lra_vcf_long_enough(INT64_MIN + 1, 1) && !lra_vcf_long_enough(2, 3) && lra_vcf_long_enough(-3, 3) && lra_vcf_long_enough(3, 3));

  // the refusal's order
  for (int it = 0; it < 100000; it++) {
    unsigned long long res[LRA_VCF_BAD_KINDS];
    const uint64_t lim = g() % 50;
    uint64_t lowest = ~0ull; int kind = -1;
    for (int k = 0; k < LRA_VCF_BAD_KINDS; k++) {
      res[k] = g() % 3 ? ~0ull : g() % 60;
      if (res[k] < lim && res[k] < lowest) { lowest = res[k]; kind = k; }
    }
    uint64_t idx = 12345; int got = -7;
    const bool any = lra_vcf_first_bad(res, lim, &idx, &got);
    CHECK(any == (kind >= 0));
    if (any) CHECK(idx == lowest && got == kind && strlen(lra_vcf_bad_text(got)) > 10); else CHECK(idx == 12345 && got == -7);
  }

  // the options
  lra_vcf_rules r = lra_vcf_rules_of(1, ~0u, 7, 0, 5);
  CHECK(r.require == 1 && r.exclude == 4 && r.min_mapq == 7 && r.min_length == 1 && r.pos_one_based == 1);
  r = lra_vcf_rules_of(0, 0, 0, 50, 0);
  CHECK(r.exclude == 0 && r.min_length == 50 && r.pos_one_based == 0);

  // a piece's bytes
  uint64_t a, b, c;
  CHECK(lra_vcf_piece_bytes(3, 1000, 1, 1, &a, &b, &c) && a == 1064 && b == 1001 && c == 120);
  CHECK(lra_vcf_piece_bytes(3, 1000, 0, 1, &a, &b, &c) && a == 0 && b == 0 && c == 120);
  CHECK(lra_vcf_piece_bytes(3, 1000, 1, 0, &a, &b, &c) && a == 1064 && c == 0);
  CHECK(lra_vcf_piece_bytes(1, 5ull << 32, 1, 0, &a, &b, &c) && a == (5ull << 32) + 64);       // beyond 32 bits is no wrap
  CHECK(!lra_vcf_piece_bytes(1, UINT64_MAX - 10, 1, 0, &a, &b, &c) && !lra_vcf_piece_bytes(UINT64_MAX / 8, 10, 1, 1, &a, &b, &c));

  // the tables
  std::string why;
  CHECK(lra_vcf_table_diff({0, 10, 30}, 30, {10, 20}, &why) == -1);
  CHECK(lra_vcf_table_diff({0, 10, 30}, 30, {10, 21}, &why) == 1 && why.find("21 bases in the BAM header and 20 in the genome") != std::string::npos);
  CHECK(lra_vcf_table_diff({0, 10, 30}, 30, {11, 21}, &why) == 0);
  CHECK(lra_vcf_table_diff({0, 10, 30}, 30, {10}, &why) == 1 && lra_vcf_table_diff({0, 10}, 10, {10, 20}, &why) == 1 && why.find("2 references") != std::string::npos);
  CHECK(lra_vcf_table_diff({}, 0, {10}, &why) == 0 && lra_vcf_table_diff({0, 10, 30}, 29, {10, 20}, &why) == 2 && lra_vcf_table_diff({}, 0, {}, &why) == -1);
  CHECK(lra_vcf_table_diff({0, 10, 5}, 30, {10, 0}, &why) == -1);                                // (a table that descends reads as length 0: no index leaves the vector)

  if (fails) printf("bam_vcf_host_check: %d checks FAILED\n", fails);
  else printf("bam_vcf_host_check: clean (%llu variants walked, %llu kept)\n", (unsigned long long)n_var, (unsigned long long)n_kept);
  return fails ? 1 : 0;
}

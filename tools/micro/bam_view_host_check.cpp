// tools/micro/bam_view_host_check.cpp -- the host parts of lra_bam_view (lra_amd/csrc/bam_view_host.h) under the host sanitizers, as a program of its own:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I lra_amd/csrc tools/micro/bam_view_host_check.cpp -o /tmp/view_check && /tmp/view_check
// A sorted record stream over three references and refID -1 is indexed by lra_bam_index_host's serial walk.  The reader takes the index whole, cut at
// every length, and with every 32-bit word of it replaced by a negative, a huge and a small count -- always from a heap block of exactly the bytes
// given, so a read one byte past them is an error here.  A whole index must plan 2000 regions ascending and disjoint, with the virtual offset of every
// record a brute-force walk finds inside a planned chunk; a damaged one must either be refused or plan without leaving its bytes.
#include "bam_view_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <random>

static void put32(std::vector<uint8_t>& o, uint32_t v) { for (int k = 0; k < 4; k++) o.push_back((uint8_t)(v >> (8 * k))); }

struct Rec { uint64_t at; int32_t ref, pos; uint64_t end; };

static uint32_t reg2bin(uint64_t beg, uint64_t end) {
  end--;
  if (beg >> 14 == end >> 14) return 4681 + (uint32_t)(beg >> 14);
  if (beg >> 17 == end >> 17) return 585 + (uint32_t)(beg >> 17);
  if (beg >> 20 == end >> 20) return 73 + (uint32_t)(beg >> 20);
  if (beg >> 23 == end >> 23) return 9 + (uint32_t)(beg >> 23);
  if (beg >> 26 == end >> 26) return 1 + (uint32_t)(beg >> 26);
  return 0;
}

static void add(std::vector<uint8_t>& o, std::vector<Rec>& R, std::mt19937_64& g, int32_t ref, int32_t pos, uint32_t span) {
  Rec r; r.at = o.size(); r.ref = ref; r.pos = pos; r.end = (uint64_t)pos + span;
  const uint32_t l_name = 1 + (uint32_t)(g() % 40), l_seq = (uint32_t)(g() % 300), bin = ref < 0 ? 4680 : reg2bin((uint64_t)pos, r.end);
  put32(o, 32 + l_name + 4 + (l_seq + 1) / 2 + l_seq);
  put32(o, (uint32_t)ref); put32(o, (uint32_t)pos);
  o.push_back((uint8_t)l_name); o.push_back(60); o.push_back((uint8_t)bin); o.push_back((uint8_t)(bin >> 8));
  o.push_back(1); o.push_back(0); o.push_back(0); o.push_back(0);
  put32(o, l_seq); put32(o, 0xffffffffu); put32(o, 0xffffffffu); put32(o, 0);
  for (uint32_t k = 0; k + 1 < l_name; k++) o.push_back('a');
  o.push_back(0);
  put32(o, span << 4);                                       // <span>M
  o.resize(o.size() + (l_seq + 1) / 2 + l_seq, 0x11);
  R.push_back(r);
}

// the reader and the planner over a heap block of exactly n bytes; -1: refused
static int run(const uint8_t* b, size_t n, int n_ref, int64_t ref, int64_t beg, int64_t end, std::vector<lra_bai_chunk>& plan) {
  uint8_t* exact = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(exact, b, n);
  std::string why;
  const int rc = lra_bai_query(n ? exact : nullptr, n, n_ref, ref, beg, end, plan, why);
  free(exact);
  if (rc && why.empty()) { fprintf(stderr, "a refusal without a reason\n"); exit(1); }
  return rc;
}

int main() {
  std::mt19937_64 g(20240611);
  const std::vector<uint64_t> ref_len = {400000, 1ull << 27, 250000};
  std::vector<uint8_t> s; std::vector<Rec> R;
  for (int32_t ref = 0; ref < 3; ref++) {
    if (ref == 2) continue;                                  // a reference without records
    std::vector<std::pair<int32_t, uint32_t>> at;
    for (int i = 0; i < 1500; i++) {
      const uint32_t span = 1 + (uint32_t)(g() % (i % 50 ? 3000 : 200000));
      at.push_back({(int32_t)(g() % (ref_len[ref] - span)), span});
    }
    if (ref == 1) at.push_back({(1 << 26) - 700, 1500});     // bin 0
    std::sort(at.begin(), at.end());
    for (auto& a : at) add(s, R, g, ref, a.first, a.second);
  }
  for (int i = 0; i < 50; i++) add(s, R, g, -1, -1, 1);
  const uint64_t n_members = (s.size() + LRA_BAI_MEMBER - 1) / LRA_BAI_MEMBER;
  std::vector<uint64_t> moff(n_members + 1);
  for (uint64_t m = 0; m <= n_members; m++) moff[m] = 20000 * m + (m * m) % 977;
  uint64_t len = 0;
  if (lra_bai_index(s.data(), s.size(), 3, ref_len.data(), moff.data(), n_members, 100, nullptr, 0, &len)) { fprintf(stderr, "the index walk refused the stream\n"); return 1; }
  std::vector<uint8_t> bai(len);
  if (lra_bai_index(s.data(), s.size(), 3, ref_len.data(), moff.data(), n_members, 100, bai.data(), len, &len)) return 1;

  std::vector<lra_bai_chunk> plan;
  size_t hits = 0;
  for (int q = 0; q < 2000; q++) {
    const int64_t ref = (int64_t)(g() % 3);
    int64_t beg = (int64_t)(g() % ref_len[ref]);
    if (q % 2) { const Rec& r = R[g() % R.size()]; if (r.ref == ref) beg = std::max<int64_t>(0, r.pos - (int64_t)(g() % 20000)); }
    const int64_t end = std::min<int64_t>((int64_t)ref_len[ref], beg + 1 + (int64_t)(g() % (1ull << (1 + g() % 27))));
    if (run(bai.data(), bai.size(), 3, ref, beg, end, plan)) { fprintf(stderr, "region %d refused\n", q); return 1; }
    for (size_t i = 0; i < plan.size(); i++)
      if (plan[i].beg >= plan[i].end || (i && plan[i - 1].end >= plan[i].beg)) { fprintf(stderr, "region %d: the plan is not ascending and disjoint\n", q); return 1; }
    for (const Rec& r : R) {
      if (r.ref != ref || r.pos >= end || (int64_t)r.end <= beg) continue;
      const uint64_t v = lra_bai_voff(r.at, moff.data(), 100);
      bool in = false;
      for (const lra_bai_chunk& c : plan) in = in || (c.beg <= v && v < c.end);
      if (!in) { fprintf(stderr, "region %d: a record at %llu is outside the plan\n", q, (unsigned long long)r.at); return 1; }
      hits++;
    }
  }
  if (run(bai.data(), bai.size(), 3, 2, 0, 250000, plan) || !plan.empty()) { fprintf(stderr, "a reference without records has a plan\n"); return 1; }
  if (run(bai.data(), bai.size(), 3, 1, (1 << 26) - 1, (1 << 26) + 1, plan) || plan.empty()) { fprintf(stderr, "the record of bin 0 is not planned\n"); return 1; }
  if (!run(bai.data(), bai.size(), 2, 0, 0, 10, plan) || !run(bai.data(), bai.size(), 3, 3, 0, 10, plan) || !run(bai.data(), bai.size(), 3, 0, 10, 9, plan)) {
    fprintf(stderr, "another n_ref, a reference outside the index or beg > end was accepted\n"); return 1;
  }
  // cut at every length: only the whole index and the one without n_no_coor are indexes
  size_t refused = 0;
  for (size_t n = 0; n < bai.size(); n++) {
    const int rc = run(bai.data(), n, 3, 0, 1000, 200000, plan);
    if ((rc == 0) != (n == bai.size() - 8)) { fprintf(stderr, "the index cut to %zu bytes: %s\n", n, rc ? "refused" : "accepted"); return 1; }
    refused += rc != 0;
  }
  // every word replaced: refused, or planned inside the bytes
  const uint32_t vals[4] = {0xffffffffu, 0x80000000u, 0x7fffffffu, 3};
  size_t damaged_ok = 0;
  for (size_t w = 0; w + 4 <= bai.size(); w += 4)
    for (uint32_t v : vals) {
      std::vector<uint8_t> d = bai;
      for (int k = 0; k < 4; k++) d[w + k] = (uint8_t)(v >> (8 * k));
      damaged_ok += run(d.data(), d.size(), 3, 0, 1000, 200000, plan) == 0;
    }
  std::vector<uint8_t> more = bai; more.push_back(0);
  if (!run(more.data(), more.size(), 3, 0, 0, 10, plan)) { fprintf(stderr, "bytes behind n_no_coor were accepted\n"); return 1; }
  printf("bam_view_host_check ok: %zu records, an index of %zu bytes, %zu overlaps inside their plans, %zu cuts refused, %zu damaged indexes still planned\n", R.size(),
         bai.size(), hits, refused, damaged_ok);
  return 0;
}

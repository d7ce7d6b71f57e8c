// tools/micro/bam_index_host_check.cpp -- lra_bam_index_host's body (lra_amd/csrc/bam_index_host.h) under the host sanitizers, as a program of its own:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I lra_amd/csrc tools/micro/bam_index_host_check.cpp -o /tmp/bai_check && /tmp/bai_check
// Every buffer the function reads or writes is a heap block of exactly its size, so a byte read or written outside one stops the run.  The streams: random
// sorted records over three references and refID -1 (records that end on a member cut, records longer than two members, 60000 ops), the empty stream, a
// stream cut short at every one of its last 40 bytes, and a reference above 2^29 bases.
#include "bam_index_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <random>

static void put32(std::vector<uint8_t>& o, uint32_t v) { for (int k = 0; k < 4; k++) o.push_back((uint8_t)(v >> (8 * k))); }

struct Rec { int32_t ref, pos; uint32_t flag; std::vector<uint8_t> bytes; };

static Rec make(std::mt19937_64& g, int32_t ref, int32_t pos, uint32_t n_ops, uint32_t l_seq, uint32_t bin) {
  Rec r; r.ref = ref; r.pos = pos; r.flag = (uint32_t)(g() & 16) | ((g() % 20 == 0) ? 4u : 0u);
  const uint32_t l_name = 1 + (uint32_t)(g() % 254);
  std::vector<uint8_t>& o = r.bytes;
  put32(o, 32 + l_name + 4 * n_ops + (l_seq + 1) / 2 + l_seq);
  put32(o, (uint32_t)ref); put32(o, (uint32_t)pos);
  o.push_back((uint8_t)l_name); o.push_back(60); o.push_back((uint8_t)bin); o.push_back((uint8_t)(bin >> 8));
  o.push_back((uint8_t)n_ops); o.push_back((uint8_t)(n_ops >> 8)); o.push_back((uint8_t)r.flag); o.push_back((uint8_t)(r.flag >> 8));
  put32(o, l_seq); put32(o, 0xffffffffu); put32(o, 0xffffffffu); put32(o, 0);
  for (uint32_t k = 0; k + 1 < l_name; k++) o.push_back('a');
  o.push_back(0);
  for (uint32_t k = 0; k < n_ops; k++) put32(o, (uint32_t)((1 + g() % 5) << 4) | (uint32_t)(g() % 9));
  o.resize(o.size() + (l_seq + 1) / 2 + l_seq, 0x11);
  return r;
}

static int index_exact(const std::vector<uint8_t>& s, const std::vector<uint64_t>& ref_len, std::vector<uint8_t>& bai) {
  const uint64_t n_members = (s.size() + LRA_BAI_MEMBER - 1) / LRA_BAI_MEMBER;
  uint8_t* stream = (uint8_t*)malloc(s.size() ? s.size() : 1);                  // exact sizes: the sanitizer watches the bytes around them
  if (s.size()) memcpy(stream, s.data(), s.size());
  uint64_t* rl = (uint64_t*)malloc(8 * (ref_len.size() ? ref_len.size() : 1));
  for (size_t i = 0; i < ref_len.size(); i++) rl[i] = ref_len[i];
  uint64_t* moff = (uint64_t*)malloc(8 * (n_members + 1));
  for (uint64_t i = 0; i <= n_members; i++) moff[i] = 1000 + 777 * i;
  uint64_t need = 0;
  int rc = lra_bai_index(s.size() ? stream : nullptr, s.size(), (int)ref_len.size(), rl, moff, n_members, 4711, nullptr, 0, &need);
  if (!rc) {
    uint8_t* out = (uint8_t*)malloc(need);
    uint64_t got = 0;
    rc = lra_bai_index(s.size() ? stream : nullptr, s.size(), (int)ref_len.size(), rl, moff, n_members, 4711, out, need, &got);
    if (!rc && got != need) rc = 99;
    if (!rc && need > 1 && lra_bai_index(s.size() ? stream : nullptr, s.size(), (int)ref_len.size(), rl, moff, n_members, 4711, out, need - 1, &got) != -1) rc = 98;
    bai.assign(out, out + need);
    free(out);
  }
  free(stream); free(rl); free(moff);
  return rc;
}

int main() {
  std::mt19937_64 g(12345);
  const std::vector<uint64_t> ref_len = {3000000, 70000, 1ull << 29};
  std::vector<Rec> recs;
  for (int i = 0; i < 3000; i++) {
    const int32_t ref = (int32_t)(g() % 4) - 1;
    if (ref < 0) { recs.push_back(make(g, -1, -1, 0, (uint32_t)(g() % 300), 4680)); continue; }
    const uint32_t n_ops = i == 7 ? 60000 : (uint32_t)(g() % 200);
    const int32_t pos = (int32_t)(g() % (ref_len[ref] - 400000 < ref_len[ref] ? (ref_len[ref] > 400000 ? ref_len[ref] - 400000 : 1000) : 1000));
    recs.push_back(make(g, ref, pos, n_ops, i % 500 == 3 ? 100000 : (uint32_t)(g() % 500), (uint32_t)(g() % 37450)));
  }
  std::stable_sort(recs.begin(), recs.end(), [](const Rec& a, const Rec& b) {
    if ((uint32_t)a.ref != (uint32_t)b.ref) return (uint32_t)a.ref < (uint32_t)b.ref;
    if (a.pos != b.pos) return a.pos < b.pos;
    return (a.flag & 16) < (b.flag & 16);
  });
  std::vector<uint8_t> s;
  for (Rec& r : recs) {
    if (s.size() < LRA_BAI_MEMBER && s.size() + r.bytes.size() > LRA_BAI_MEMBER && r.ref >= 0) {   // make one record end exactly on the first cut
      const size_t want = LRA_BAI_MEMBER - s.size();
      if (want >= 40 + 300 && r.bytes.size() > want) continue;
    }
    s.insert(s.end(), r.bytes.begin(), r.bytes.end());
  }
  std::vector<uint8_t> bai, none;
  int rc = index_exact(s, ref_len, bai);
  if (rc) { printf("FAIL: the random stream: %d\n", rc); return 1; }
  printf("random stream: %zu bytes, %zu members, .bai %zu bytes\n", s.size(), (size_t)((s.size() + LRA_BAI_MEMBER - 1) / LRA_BAI_MEMBER), bai.size());
  if (index_exact(none, ref_len, bai) || bai.size() != 8 + 3 * 8 + 8) { printf("FAIL: the empty stream\n"); return 1; }
  if (index_exact(none, {}, bai) || bai.size() != 16) { printf("FAIL: no references\n"); return 1; }
  for (size_t cut = 1; cut <= 40; cut++) {
    std::vector<uint8_t> t(s.begin(), s.end() - cut);
    if (index_exact(t, ref_len, bai) != -1) { printf("FAIL: a stream cut short by %zu bytes was taken\n", cut); return 1; }
  }
  if (index_exact(s, {3000000, 70000, (1ull << 29) + 1}, bai) != -1) { printf("FAIL: a reference above 2^29 bases was taken\n"); return 1; }
  printf("ok\n");
  return 0;
}

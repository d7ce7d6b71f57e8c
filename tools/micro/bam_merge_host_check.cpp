// tools/micro/bam_merge_host_check.cpp -- the host parts of lra_bam_merger (lra_amd/csrc/bam_merge_host.h) under the host sanitizers, as a program of its own:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I lra_amd/csrc tools/micro/bam_merge_host_check.cpp -o /tmp/merge_check && /tmp/merge_check
// A sorted record stream over three references and refID -1 is cut into rounds at random records.  Per round the program computes, serially, what the
// merger's index kernels leave (chunk heads against the last record of the round before, the chunks' [ubeg, uend) and the open end, per reference first /
// last / counters, the windows' minima, all in stream offsets); lra_merge_add_round coalesces, lra_merge_index_arrays converts with the member table, and
// the bytes lra_bai_write makes of it must be lra_bam_index_host's for the same stream -- for 1, 2, 7 and 400 rounds, the empty stream included.  The
// header parser runs over a header cut short at every length.  The member table, the counters and the header are heap blocks of exactly their size.
#include "bam_merge_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <random>

static void put32(std::vector<uint8_t>& o, uint32_t v) { for (int k = 0; k < 4; k++) o.push_back((uint8_t)(v >> (8 * k))); }

struct Rec { uint64_t at, next; int32_t ref, pos; uint32_t span, bin, flag; };

static void add(std::vector<uint8_t>& o, std::vector<Rec>& R, std::mt19937_64& g, int32_t ref, int32_t pos, uint32_t n_ops, uint32_t l_seq) {
  Rec r; r.at = o.size(); r.ref = ref; r.pos = pos; r.flag = (uint32_t)(g() & 16) | ((g() % 20 == 0) ? 4u : 0u);
  r.bin = ref < 0 ? 4680 : 4681 + (uint32_t)(pos >> 14) % 3 * (uint32_t)(g() % 2);   // (any bin will do: the index files a record under its own field)
  const uint32_t l_name = 1 + (uint32_t)(g() % 40);
  put32(o, 32 + l_name + 4 * n_ops + (l_seq + 1) / 2 + l_seq);
  put32(o, (uint32_t)ref); put32(o, (uint32_t)pos);
  o.push_back((uint8_t)l_name); o.push_back(60); o.push_back((uint8_t)r.bin); o.push_back((uint8_t)(r.bin >> 8));
  o.push_back((uint8_t)n_ops); o.push_back((uint8_t)(n_ops >> 8)); o.push_back((uint8_t)r.flag); o.push_back((uint8_t)(r.flag >> 8));
  put32(o, l_seq); put32(o, 0xffffffffu); put32(o, 0xffffffffu); put32(o, 0);
  for (uint32_t k = 0; k + 1 < l_name; k++) o.push_back('a');
  o.push_back(0);
  uint64_t span = 0;
  for (uint32_t k = 0; k < n_ops; k++) {
    const uint32_t op = (uint32_t)((1 + g() % 3000) << 4) | (uint32_t)(g() % 9);
    put32(o, op);
    if ((0x18du >> (op & 15)) & 1) span += op >> 4;
  }
  r.span = (uint32_t)std::max<uint64_t>(span, 1);
  o.resize(o.size() + (l_seq + 1) / 2 + l_seq, 0x11);
  r.next = o.size();
  R.push_back(r);
}

static int check(const std::vector<uint8_t>& s, const std::vector<Rec>& R, const std::vector<uint64_t>& ref_len, size_t n_rounds, std::mt19937_64& g) {
  const uint64_t first = 4711, n_members = (s.size() + LRA_BAI_MEMBER - 1) / LRA_BAI_MEMBER;
  const int n_ref = (int)ref_len.size();
  uint64_t* moff = (uint64_t*)malloc(8 * (n_members + 1));
  for (uint64_t i = 0; i <= n_members; i++) moff[i] = 1000 + 777 * i;
  uint64_t need = 0;
  if (lra_bai_index(s.data(), s.size(), n_ref, ref_len.data(), moff, n_members, first, nullptr, 0, &need)) return 1;
  std::vector<uint8_t> want(need);
  if (lra_bai_index(s.data(), s.size(), n_ref, ref_len.data(), moff, n_members, first, want.data(), need, &need)) return 2;
  // the rounds
  std::vector<size_t> cut{0, R.size()};
  for (size_t i = 1; i < n_rounds && R.size(); i++) cut.push_back((size_t)(g() % (R.size() + 1)));
  std::sort(cut.begin(), cut.end());
  std::vector<uint64_t> lin_off((size_t)n_ref + 1, 0);
  for (int r = 0; r < n_ref; r++) lin_off[(size_t)r + 1] = lin_off[r] + lra_bai_windows(ref_len[r]);
  std::vector<uint64_t> lin(lin_off[n_ref], LRA_BAI_NONE);
  unsigned long long* stat = (unsigned long long*)calloc(5 * (size_t)n_ref + 1, 8);
  for (int r = 0; r < n_ref; r++) stat[5 * r] = LRA_BAI_NONE;
  std::vector<lra_merge_chunk> C;
  int32_t c_ref = -1; uint32_t c_bin = 0;
  for (size_t q = 0; q + 1 < cut.size(); q++) {
    const size_t a = cut[q], b = cut[q + 1];
    if (a == b) continue;                                       // (a round always holds a record)
    std::vector<uint64_t> key, beg, end;
    uint64_t open_end = LRA_BAI_NONE;
    for (size_t p = a; p < b; p++) {
      const Rec& r = R[p];
      if (r.ref < 0) { stat[5 * n_ref]++; continue; }
      const int32_t pref = p > a ? R[p - 1].ref : c_ref;
      const uint32_t pbin = p > a ? R[p - 1].bin : c_bin;
      const bool head = pref != r.ref || pbin != r.bin;
      if (head) { key.push_back(((uint64_t)(uint32_t)r.ref << 16) | r.bin); beg.push_back(r.at); end.push_back(0); }
      const bool last = p + 1 == b || R[p + 1].ref < 0 || R[p + 1].ref != r.ref || R[p + 1].bin != r.bin;
      if (last) { if (key.empty()) open_end = r.next; else end.back() = r.next; }
      unsigned long long* S = stat + 5 * r.ref;
      S[0] = std::min<unsigned long long>(S[0], r.at); S[1] = std::max<unsigned long long>(S[1], r.next); S[(r.flag & 4) ? 3 : 2]++;
      const uint64_t n_win = lin_off[r.ref + 1] - lin_off[r.ref], p0 = r.pos < 0 ? 0 : (uint64_t)r.pos;
      const uint64_t w0 = std::min(p0 >> 14, n_win - 1), w1 = std::min((p0 + r.span - 1) >> 14, n_win - 1);
      for (uint64_t w = w0; w <= w1; w++) { uint64_t& x = lin[lin_off[r.ref] + w]; x = std::min(x, r.at); }
      S[4] = std::max<unsigned long long>(S[4], w1 + 1);
    }
    lra_merge_add_round(C, open_end, key.data(), beg.data(), end.data(), key.size());
    c_ref = R[b - 1].ref < 0 ? -1 : R[b - 1].ref; c_bin = R[b - 1].bin;
  }
  std::vector<uint32_t> order(C.size());
  for (size_t i = 0; i < C.size(); i++) order[i] = (uint32_t)i;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return C[x].key < C[y].key; });   // (references ascend in file order: by (ref, bin), stable)
  lra_bai_arrays A;
  lra_merge_index_arrays(C, order, stat, lin, lin_off, moff, first, A);
  std::vector<uint8_t> got;
  lra_bai_write(A, got);
  free(moff); free(stat);
  return got == want ? 0 : 3;
}

int main() {
  std::mt19937_64 g(7);
  const std::vector<uint64_t> ref_len{400000, 300000, 250000};
  std::vector<uint8_t> s; std::vector<Rec> R;
  for (int ref = 0; ref < 3; ref++) {
    int32_t pos = 0;
    for (int i = 0; i < 700; i++) {
      pos += (int32_t)(g() % 3 ? 0 : g() % 900);                // many ties
      add(s, R, g, ref, pos, (uint32_t)(g() % 30), (uint32_t)(g() % 300));
    }
  }
  for (int i = 0; i < 200; i++) add(s, R, g, -1, -1, 0, (uint32_t)(g() % 300));
  for (size_t rounds : {(size_t)1, (size_t)2, (size_t)7, (size_t)400})
    for (int rep = 0; rep < 4; rep++)
      if (int rc = check(s, R, ref_len, rounds, g)) { printf("FAIL: %zu rounds, code %d\n", rounds, rc); return 1; }
  if (int rc = check(std::vector<uint8_t>(), std::vector<Rec>(), ref_len, 1, g)) { printf("FAIL: the empty stream, code %d\n", rc); return 1; }
  // the header's reference table, whole and cut short at every length
  std::vector<uint8_t> h{'B', 'A', 'M', 1};
  put32(h, 5); for (char c : std::string("@HD\t\n")) h.push_back((uint8_t)c);
  put32(h, 3);
  for (int i = 0; i < 3; i++) { put32(h, 5); for (char c : std::string("chr")) h.push_back((uint8_t)c); h.push_back((uint8_t)('1' + i)); h.push_back(0); put32(h, (uint32_t)ref_len[i]); }
  for (size_t n = 0; n <= h.size(); n++) {
    uint8_t* b = (uint8_t*)malloc(n ? n : 1);
    memcpy(b, h.data(), n);
    lra_merge_refs T;
    const bool ok = lra_merge_parse_refs(b, n, T);
    free(b);
    if (ok != (n == h.size())) { printf("FAIL: a header of %zu of %zu bytes\n", n, h.size()); return 1; }
    if (ok && (T.n_ref != 3 || T.name[2] != "chr3" || T.len[1] != 300000)) { printf("FAIL: the table\n"); return 1; }
  }
  printf("bam_merge_host_check ok: %zu records, %zu bytes\n", R.size(), s.size());
  return 0;
}

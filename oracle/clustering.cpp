// oracle/clustering.cpp -- TEST INFRASTRUCTURE ONLY (see oracle_common.h).
//
// CPU restatement of CleanMatches (reference: Clustering.h:1840-1906) as every preset runs it
// (opts.ExtractDiagonalFromClean == true): DiagonalSort / AntiDiagonalSort (Sorting.h:50-68,
// 113-136), CleanOffDiagonal (Clustering.h:566-798), AVGfreq (:550-564),
// SecondRoundCleanOffDiagonal (:802-868), Cluster boundaries (:308-322), chromIndex
// (Genome.h:20-32).
// Parity status: PARITY UNPINNED -- Clustering.h needs Genome (-> htslib/kseq.h, absent), so it
// cannot be compiled here; restated from the source text.
#include "oracle_common.h"
#include "../include/lra_hip.h"
#include <algorithm>
#include <cmath>
#include <unordered_map>
#include <vector>

// Hit counts of the branches below, for the tests that must know which of them their inputs reach (tests/oracle_lib.py: CLEAN_COUNTERS names the slots).
enum {
  CC_NO_NEIGHBOUR, CC_MINDIAG_ZERO, CC_RUN_TOO_SHORT,
  CC_BYPASS_DROP, CC_BYPASS_GE2, CC_BYPASS_GE1_5, CC_BYPASS_KEEP,
  CC_DROP, CC_GE4, CC_GE1_5, CC_GT1_LONG, CC_GT1_SHORT, CC_KEEP,
  CC_SR_EXIT_GE_LEN, CC_SR_EXIT_LE_ZERO, CC_SR_EXIT_ONE_MATCH,
  CC_SR_NONE_LONG, CC_SR_ONE_LONG, CC_SR_SEVERAL_LONG, CC_SR_INNER_SPAN,
  CC_N
};
static long g_clean_hits[CC_N];

namespace {
struct M { uint32_t q, t; uint64_t key; };

long diag_diff(const M& a, const M& b, int strand) {                    // Clustering.h:503-514
  if (strand == 0) return ((long)a.t - (long)a.q) - ((long)b.t - (long)b.q);
  return (long)(uint32_t)(a.q + a.t) - (long)(uint32_t)(b.q + b.t);   // 32-bit sums, as `long aDiag = a.first.pos + a.second.pos`
}

int header_find(const uint64_t* pos, int npos, uint64_t query) {         // Genome.h:20-32 (pos has nchrom+1 entries)
  if (npos > 0 && query == pos[0]) return 0;
  const uint64_t* it = std::lower_bound(pos, pos + npos, query);
  int i = (int)(it - pos);
  if (it != pos + npos && query == *it) return i;
  return i - 1;
}

void second_round(std::vector<int>& count, int out_counter, std::vector<M>& m, int MinDiagCluster, int CleanMaxDiag,
                  std::vector<char>& orig, int os, int oe, int strand) { // :802-868
  if (MinDiagCluster >= oe - os) { g_clean_hits[CC_SR_EXIT_GE_LEN]++; return; }
  if (MinDiagCluster <= 0) { g_clean_hits[CC_SR_EXIT_LE_ZERO]++; for (int i = os; i < oe; i++) { orig[i] = 1; count[i] = out_counter; } return; }
  if (oe - os <= 1) { g_clean_hits[CC_SR_EXIT_ONE_MATCH]++; return; }
  std::vector<char> fw(oe - os, 0), rv(oe - os, 0);
  for (int i = os + 1; i < oe; i++) if (std::labs(diag_diff(m[i], m[i - 1], strand)) < CleanMaxDiag) fw[i - 1 - os] = 1;
  {                                                                      // (counters only) the sub-runs that are long enough, before the passes rewrite the flags
    int nlong = 0, open = -1;
    for (int i = os; i < oe; i++) {
      if (open < 0 && fw[i - os]) open = i;
      else if (open >= 0 && !fw[i - os]) { if (i - open + 1 >= MinDiagCluster) nlong++; open = -1; }
    }
    g_clean_hits[nlong == 0 ? CC_SR_NONE_LONG : nlong == 1 ? CC_SR_ONE_LONG : CC_SR_SEVERAL_LONG]++;
  }
  bool prev = false; int ds = 0;
  for (int i = os; i < oe; i++) {
    if (!prev && fw[i - os]) ds = i;
    if (prev && !fw[i - os]) {
      if (i - ds + 1 < MinDiagCluster) { for (int j = ds; j <= i; j++) fw[j - os] = 0; }
      else fw[i - os] = 1;
    }
    prev = fw[i - os];
  }
  for (int i = oe - 2; i >= os; i--) if (std::labs(diag_diff(m[i], m[i + 1], strand)) < CleanMaxDiag) rv[i + 1 - os] = 1;
  prev = false;
  for (int i = oe - 1; i >= os; i--) {
    if (!prev && rv[i - os]) ds = i;
    if (prev && !rv[i - os]) {
      if (ds - i + 1 < MinDiagCluster) { for (int j = i; j <= ds; j++) rv[j - os] = 0; }
      else rv[i - os] = 1;
    }
    prev = rv[i - os];
  }
  for (int i = os; i < oe; i++) {
    if (fw[i - os] && rv[i - os]) { orig[i] = 1; count[i] = out_counter; }
    else orig[i] = 0;
  }
  int first = -1, last = -1;
  for (int i = os; i < oe; i++) if (orig[i]) { if (first < 0) first = i; last = i; }
  if (first > os && last >= 0 && last < oe - 1) g_clean_hits[CC_SR_INNER_SPAN]++;
}
}  // namespace

// the hit counts since the last reset (CC_N slots)
extern "C" int oracle_clean_counters(long* out, int reset) {
  if (out) for (int i = 0; i < CC_N; i++) out[i] = g_clean_hits[i];
  if (reset) for (int i = 0; i < CC_N; i++) g_clean_hits[i] = 0;
  return CC_N;
}

// One strand of one read.  Inputs: the matches (read pos, genome pos, read minimizer key incl. strand
// bit).  Outputs: cleaned sorted matches (out_q/out_t, capacity n) and clusters (capacity n each).
// Returns the number of clusters; *n_clean the number of surviving matches.
extern "C" long oracle_clean_matches(const uint32_t* qpos, const uint32_t* tpos, const uint64_t* qkey, long n, int strand,
                                     const lra_clean_opts* o, const uint64_t* chrom_pos, int n_chrom, uint32_t* out_q,
                                     uint32_t* out_t, long* n_clean, long* c_start, long* c_end, uint32_t* c_qs, uint32_t* c_qe,
                                     uint32_t* c_ts, uint32_t* c_te, int* c_chrom, float* c_freq) {
  *n_clean = 0;
  if (n == 0) return 0;                                                  // :568-570
  std::vector<M> m(n);
  for (long i = 0; i < n; i++) m[i] = {qpos[i], tpos[i], qkey[i]};
  if (strand == 0)                                                       // Sorting.h:34-47
    std::sort(m.begin(), m.end(), [](const M& a, const M& b) {
      long ad = (long)a.q - (long)a.t, bd = (long)b.q - (long)b.t;
      return ad != bd ? ad < bd : a.q < b.q;
    });
  else                                                                   // Sorting.h:74-88 (32-bit sum)
    std::sort(m.begin(), m.end(), [](const M& a, const M& b) {
      uint32_t ad = a.q + a.t, bd = b.q + b.t;
      return ad != bd ? ad < bd : a.q < b.q;
    });
  std::vector<float> freq(n, 1.0f);
  std::vector<char> onDiag(n, 0);
  if (n > 1 && std::labs(diag_diff(m[0], m[1], strand)) < o->cleanMaxDiag) onDiag[0] = 1;            // :573-576
  for (long i = 1; i < n; i++) if (std::labs(diag_diff(m[i], m[i - 1], strand)) < o->cleanMaxDiag) onDiag[i - 1] = 1;   // :578-584
  bool prev = false, startSet = false;
  int diagStart = 0, largest = 0;
  for (long i = 0; i < n; i++) {                                         // :589-598
    if (!prev && onDiag[i]) { diagStart = (int)i; startSet = true; }
    if (prev && !onDiag[i]) largest = std::max(largest, (int)i - diagStart + 1);
    prev = onDiag[i];
  }
  if (!startSet) { g_clean_hits[CC_NO_NEIGHBOUR]++; return 0; }          // :600-603
  largest = std::max(largest, (int)n - diagStart);
  int minDiagCluster = (int)std::floor(largest / 10);                    // :608-609
  if (minDiagCluster >= o->minDiagCluster) minDiagCluster = o->minDiagCluster;
  if (minDiagCluster == 0) g_clean_hits[CC_MINDIAG_ZERO]++;
  std::vector<int> count(n, -1);
  std::vector<char> second(n, 0);
  int counter = 0;
  prev = false;
  if (minDiagCluster >= 0) {
    for (long i = 0; i < n; i++) {                                       // :620-722
      if (!prev && onDiag[i]) diagStart = (int)i;
      if (prev && !onDiag[i]) {
        const int len = (int)i - diagStart + 1;
        if (len < minDiagCluster) {
          g_clean_hits[CC_RUN_TOO_SHORT]++;
          for (int j = diagStart; j <= i; j++) second[j] = 0;
        } else {
          std::unordered_map<uint64_t, int> mc;                          // AVGfreq :550-564
          for (int r = diagStart; r <= i; r++) mc[m[r].key]++;
          const float avgfreq = (float)(len) / mc.size();
          for (int j = diagStart; j <= i; j++) freq[j] = avgfreq;
          int MinDiagCluster = 0;
          const int cc = o->cleanClustersize;
          if (o->bypassClustering) {                                     // :635-657
            if (avgfreq >= 3.0f && len < 10) { g_clean_hits[CC_BYPASS_DROP]++; for (int j = diagStart; j <= i; j++) second[j] = 0; }
            else if (avgfreq >= 2.0f && len >= cc) {
              g_clean_hits[CC_BYPASS_GE2]++;
              MinDiagCluster = o->SecondCleanMinDiagCluster + std::floor((avgfreq - 1.5f) / 1.0f) * o->punish_anchorfreq +
                               std::floor((len - cc) / cc) * o->anchorPerlength;
              second_round(count, counter, m, MinDiagCluster, o->SecondCleanMaxDiag, second, diagStart, (int)i + 1, strand);
            } else if (avgfreq >= 1.5f && len >= cc) {
              g_clean_hits[CC_BYPASS_GE1_5]++;
              MinDiagCluster = o->SecondCleanMinDiagCluster + std::floor((avgfreq - 1.5f) / 1.5f) * o->punish_anchorfreq +
                               std::floor((len - cc) / cc) * o->anchorPerlength;
              second_round(count, counter, m, MinDiagCluster, o->SecondCleanMaxDiag, second, diagStart, (int)i + 1, strand);
            } else { g_clean_hits[CC_BYPASS_KEEP]++; for (int j = diagStart; j <= i; j++) { second[j] = 1; count[j] = counter; } }
          } else {                                                       // :659-693
            if (avgfreq >= 3.0f && len < 10) { g_clean_hits[CC_DROP]++; for (int j = diagStart; j <= i; j++) second[j] = 0; }
            else if (avgfreq >= 4.0f && len >= cc) {
              g_clean_hits[CC_GE4]++;
              MinDiagCluster = o->SecondCleanMinDiagCluster + std::floor((avgfreq - 1.5f) / 1.0f) * o->punish_anchorfreq +
                               std::floor((len - cc) / cc) * o->anchorPerlength;
              second_round(count, counter, m, MinDiagCluster, o->SecondCleanMaxDiag, second, diagStart, (int)i + 1, strand);
            } else if (avgfreq >= 1.5f && len >= cc) {
              g_clean_hits[CC_GE1_5]++;
              MinDiagCluster = o->SecondCleanMinDiagCluster + std::floor((avgfreq - 1.5f) / 1.5f) * o->punish_anchorfreq +
                               std::floor((len - cc) / cc) * o->anchorPerlength;
              second_round(count, counter, m, MinDiagCluster, o->SecondCleanMaxDiag, second, diagStart, (int)i + 1, strand);
            } else if (avgfreq > 1.0f && len >= cc) {
              g_clean_hits[CC_GT1_LONG]++;
              MinDiagCluster = o->SecondCleanMinDiagCluster - (5 - std::floor((avgfreq - 1.0f) / 0.1f)) * (o->punish_anchorfreq / 2) +
                               std::floor((len - cc) / cc) * (o->anchorPerlength / 2);
              second_round(count, counter, m, MinDiagCluster, o->SecondCleanMaxDiag, second, diagStart, (int)i + 1, strand);
            } else if (avgfreq > 1.0f) {
              g_clean_hits[CC_GT1_SHORT]++;
              MinDiagCluster = o->SecondCleanMinDiagCluster - (5 - std::floor((avgfreq - 1.0f) / 0.1f)) * (o->punish_anchorfreq / 2) -
                               std::floor((cc - (int)i + diagStart - 1) / 15) * (o->anchorPerlength / 2);
              second_round(count, counter, m, MinDiagCluster, o->SecondCleanMaxDiag, second, diagStart, (int)i + 1, strand);
            } else { g_clean_hits[CC_KEEP]++; for (int j = diagStart; j <= i; j++) { second[j] = 1; count[j] = counter; } }
          }
        }
        counter++;
      }
      prev = onDiag[i];
    }
  }
  long c = 0;
  for (long i = 0; i < n; i++)                                           // :728-738
    if (second[i]) { m[c] = m[i]; freq[c] = freq[i]; count[c] = count[i]; c++; }
  *n_clean = c;
  for (long i = 0; i < c; i++) { out_q[i] = m[i].q; out_t[i] = m[i].t; }
  // clusters (:740-797): maximal stretches of equal `count`
  long ncl = 0;
  auto emit = [&](long s, long e) {
    uint32_t qS = m[s].q, qE = m[s].q + o->globalK, tS = m[s].t, tE = m[s].t + o->globalK;
    for (long b = s; b < e; b++) {
      qS = std::min(qS, m[b].q); qE = std::max(qE, m[b].q + (uint32_t)o->globalK);
      tS = std::min(tS, m[b].t); tE = std::max(tE, m[b].t + (uint32_t)o->globalK);
    }
    c_start[ncl] = s; c_end[ncl] = e; c_qs[ncl] = qS; c_qe[ncl] = qE; c_ts[ncl] = tS; c_te[ncl] = tE;
    c_freq[ncl] = freq[s];
    c_chrom[ncl] = header_find(chrom_pos, n_chrom + 1, tS);              // :760-761 (only set when bypassClustering; reported always)
    ncl++;
  };
  long count_s = 0, cc2 = 1;
  while (cc2 < c) {
    if (count[cc2] == count[cc2 - 1]) { cc2++; continue; }
    emit(count_s, cc2);
    count_s = cc2;
    cc2++;
  }
  if (cc2 == c && count_s < cc2) emit(count_s, cc2);
  return ncl;
}

// oracle/local_refine.cpp -- TEST INFRASTRUCTURE ONLY (see oracle_common.h).
//
// CPU restatement of the chain walk that turns the chains of the second sparse DP into alignments (low-accuracy path, Map_lowacc.h:575-576):
//   LocalRefineAlignment(ultimatechains, ext_clusters, alignments, smallOpts, ..., h, genome, LSC, tinyOpts, ...)   LocalRefineAlignment.h:885-1029
//   RefinedAlignmentbtwnAnchors                                                                                      LocalRefineAlignment.h:203-550
//   RefineByLinearAlignment :141-185 (oracle_between_anchors), RefineSpace (oracle_refine_space), LinearExtend pair version
//   (oracle_linear_extend after DiagonalSort), TrimOverlappedAnchors pair version (oracle_trim_anchor_pairs), SparseDP_ForwardOnly
//   (oracle_sdp_chain, single-cluster mode on a forward cluster), RemovePairedIndels pair version (oracle_filter_chain op 5)
// Parity status: PARITY UNPINNED -- LocalRefineAlignment.h needs Genome.h / Clustering.h (htslib); restated from the source text.
// The +,-,+ / typeofaln = 3 pass at the end of the function (:997-1023) reads nm, tStart and tEnd of the new alignments, which are
// still the constructor's zeros there (CalculateStatistics runs later, Map_lowacc.h:596), so it never marks anything; restated as such.
#include "oracle_common.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

extern "C" long oracle_refine_space(const char* q, int qLen, const char* t, int tLen, uint32_t tSpan, int K, int W, int refineSpaceDiag, int match,
                                    int mismatch, int indel, long maxFreq, uint32_t qAdd, uint32_t tAdd, uint32_t flipLen, uint32_t* outQ,
                                    uint32_t* outT, long cap, float* identity);
extern "C" long oracle_linear_extend(const uint32_t* q, const uint32_t* t, long n, int strand, int K, const char* read, uint32_t readLen,
                                     const char* chrom, uint32_t chromLen, uint32_t* eq, uint32_t* et, int* elen, uint32_t* box);
extern "C" void oracle_trim_anchor_pairs(int n, const uint32_t* Q, const uint32_t* T, int* L);
extern "C" int oracle_filter_chain(int n, const uint32_t* q, const uint32_t* t, const int* len, const uint8_t* strand, const uint8_t* link, int hasLink,
                                   const int* ops, int nOps, uint8_t* keep, uint8_t* linkOut, int* nLink);
extern "C" int oracle_between_anchors(const char* q, const char* t, uint32_t curReadEnd, uint32_t nextReadStart, uint32_t curGenomeEnd,
                                      uint32_t nextGenomeStart, int match, int mismatch, int indel, int localBand, int refineDp, int* blocks, int cap,
                                      int* score);
struct oracle_sdp_opts { float rate; int NumAln; float alnthres; int readLen; float gapopen, gapextend, gaproot; int gapCeiling1, gapCeiling2; int mode; int globalK; };
extern "C" int oracle_sdp_chain(int nClusters, const int* clusterOff, const uint8_t* clusterStrand, const uint32_t* q, const uint32_t* t,
                                const int* len, const oracle_sdp_opts* o, float* fragVal, long* fragPrevSub, long* fragPrevInd,
                                uint8_t* fragFlags, int maxChains, int* chainOff, uint32_t* chainFrag, uint8_t* chainLink, uint32_t* chainBox,
                                float* chainValue);

struct oracle_lra_opts {
  int localW, globalW, localMaxFreq;     // tinyOpts.localW / globalW / localMaxFreq on entry (Map_lowacc.h:241-242: globalW = localW)
  int match, mismatch, indel, localBand; // localMatch / localMismatch / localIndel / localBand
  int refineBySDP, isOnt;                // Options::RefineBySDP; readType clr / ont (1) or contig / ccs (0)
  float gapopen, gapextend, gaproot; int gapCeiling1, gapCeiling2;   // the PWL table of the sparse DP
};

namespace {

struct Aln { int strand, supp, secondary, N0, N1, chrom; float value; std::vector<int> blocks; };   // blocks: qPos, tPos, length triples

struct Env {
  const char* strands[2]; uint32_t readLen; const char* genome; const uint64_t* chromPos; const oracle_lra_opts* o; bool bad = false;
  const char* chromSeq(int c) const { return genome + chromPos[c]; }
  uint32_t chromLen(int c) const { return (uint32_t)(chromPos[c + 1] - chromPos[c]); }
};

void linear_between(Env& E, uint32_t cre, uint32_t cge, uint32_t nrs, uint32_t ngs, int str, int chrom, Aln* a) {   // RefineByLinearAlignment :141-185
  const int cap = std::max(0, (int)(nrs - cre)) + std::max(0, (int)(ngs - cge)) + 16;
  std::vector<int> b(3 * (size_t)std::max(cap, 16));
  int score = 0;
  const int nb = oracle_between_anchors(E.strands[str], E.chromSeq(chrom), cre, nrs, cge, ngs, E.o->match, E.o->mismatch, E.o->indel, E.o->localBand, 1, b.data(),
                                        std::max(cap, 16), &score);
  if (nb < 0) { E.bad = true; return; }
  a->blocks.insert(a->blocks.end(), b.begin(), b.begin() + 3 * nb);
}

long refine_space(Env& E, int K, int W, int diag, int maxFreq, int chrom, uint32_t qe, uint32_t qs, uint32_t te, uint32_t ts, int st, std::vector<uint32_t>& oq,
                  std::vector<uint32_t>& ot, float& identity) {
  long cap = 4096;
  if ((int)(qe - qs) < 0 || (int)(te - ts) < 0) { E.bad = true; return 0; }   // a negative span: the reference hands RefineSpace a pointer and a length that do not describe a string
  for (;;) {
    oq.resize(cap); ot.resize(cap);
    const long n = oracle_refine_space(E.strands[st] + qs, (int)(qe - qs), E.chromSeq(chrom) + ts, (int)(te - ts), te - ts, K, W, diag, E.o->match, E.o->mismatch,
                                       E.o->indel, maxFreq, qs, ts, 0, oq.data(), ot.data(), cap, &identity);
    if (n < 0) { E.bad = true; return 0; }
    if (n <= cap) { oq.resize(n); ot.resize(n); return n; }
    cap = n;
  }
}

// What one anchor pair did, for the tests that have to prove which branch a crafted case took: oracle_lr_trace_fields() doubles per pair, -1 where a
// field does not apply.  The device plans more than the walk uses (every read-strand seed set, and the other strand of every space that passes
// the ratio and identity clauses of :287-289 whatever the block count); T_SUPER / T_SPEC / T_JOBS / T_NP2 restate that plan, and are computed
// only when a trace is asked for.
enum { T_CHAIN, T_CUR, T_TYPE, T_RD, T_GD, T_K, T_W, T_MF, T_DIAG, T_SV, T_NF, T_IDF, T_SUPER, T_BLOCKS, T_TRIED, T_NR, T_IDR, T_OUTCOME, T_IN_BEFORE, T_IN_AFTER,
       T_BTC_START, T_BTC_END, T_FINAL, T_RM_MAX, T_KEPT_MIN, T_SPEC, T_JOBS, T_NP2, T_N };
static_assert(T_N == 28, "tests/oracle_lib.py LR_TRACE_FIELDS");

// :295-330 as a function of the two seed sets: 0 break, 1 forward seeds, 2 inverted seeds
int decide(const oracle_lra_opts* o, size_t nf, size_t nr, float identity, int minDist, int sv_diag, float minRatio) {
  const double driftRate = o->isOnt ? 0.10f : 0.01f;
  if (nf == 0 && nr == 0 && minDist > 500 && sv_diag <= std::max((double)50, minDist * driftRate)) return 0;
  if (identity < 0.8 && nr / (float)minDist < minRatio) return 0;
  return nf >= nr ? 1 : 2;
}

// :332-472 for one seed set: LinearExtend, the boundary anchors (read-strand seeds only), TrimOverlappedAnchors, SparseDP_ForwardOnly, RemovePairedIndels,
// btc_start / btc_end.  Reads only; the caller walks the chain.
struct Inner {
  std::vector<uint32_t> chain, eq, et; std::vector<int> el; long ne = 0; float value = 0; int before = 0, bs = 0, be = -1, rmMax = -1, keptMin = -1;   // rmMax / keptMin: the longest anchor RemovePairedIndels took, the shortest it left (boundary anchors aside)
  bool sdpBad = false, fin = false; int np = 0;
};
Inner plan_inner(const Env& E, const std::vector<uint32_t>& bq, const std::vector<uint32_t>& bt, bool inversion, int K, int chrom, uint32_t curReadEnd, uint32_t curGenomeEnd,
                 uint32_t nextReadStart, uint32_t nextGenomeStart, int lenCur, int lenNext) {
  Inner I;
  const uint32_t L = E.readLen;
  // LinearExtend(BtwnPairs, ..., chromIndex, strand 0, skipsorting 0, K) on read.seq (the forward read, whatever str)
  const size_t n = bq.size();
  std::vector<std::pair<uint32_t, uint32_t>> P(n);
  for (size_t i = 0; i < n; i++) P[i] = std::make_pair(bq[i], bt[i]);
  std::sort(P.begin(), P.end(), [](const std::pair<uint32_t, uint32_t>& a, const std::pair<uint32_t, uint32_t>& b) {
    const long aD = (long)a.first - (long)a.second, bD = (long)b.first - (long)b.second;
    if (aD != bD) return aD < bD;
    return a.first < b.first;
  });
  std::vector<uint32_t> sq(n), st(n);
  I.eq.resize(n + 2); I.et.resize(n + 2); I.el.resize(n + 2);
  std::vector<uint32_t>& eq = I.eq; std::vector<uint32_t>& et = I.et; std::vector<int>& el = I.el;
  for (size_t i = 0; i < n; i++) { sq[i] = P[i].first; st[i] = P[i].second; }
  uint32_t bx[4];
  long ne = oracle_linear_extend(sq.data(), st.data(), (long)n, 0, K, E.strands[0], L, E.chromSeq(chrom), E.chromLen(chrom), eq.data(), et.data(), el.data(), bx);
  if (!inversion) {
    eq[ne] = nextReadStart; et[ne] = nextGenomeStart; el[ne] = lenNext; ne++;
    eq[ne] = curReadEnd - lenCur; et[ne] = curGenomeEnd - lenCur; el[ne] = lenCur; ne++;
  }
  I.ne = ne;
  oracle_trim_anchor_pairs((int)ne, eq.data(), et.data(), el.data());
  // SparseDP_ForwardOnly(..., rate 2) = the single-cluster sparse DP on one forward cluster; inv_value = its best value
  oracle_sdp_opts so; so.rate = 2.0f; so.NumAln = 1; so.alnthres = 0; so.readLen = (int)L; so.gapopen = E.o->gapopen; so.gapextend = E.o->gapextend;
  so.gaproot = E.o->gaproot; so.gapCeiling1 = E.o->gapCeiling1; so.gapCeiling2 = E.o->gapCeiling2; so.mode = 1; so.globalK = K;
  const int off2[2] = {0, (int)ne}; const uint8_t cst[1] = {0};
  std::vector<float> fv(ne); std::vector<int> coff(2); std::vector<uint32_t> cf(ne); std::vector<uint8_t> cl(ne); uint32_t cb[4]; float cv[1] = {0};
  const int nc = oracle_sdp_chain(1, off2, cst, eq.data(), et.data(), el.data(), &so, fv.data(), nullptr, nullptr, nullptr, 1, coff.data(), cf.data(), cl.data(), cb, cv);
  if (nc < 0) { I.sdpBad = true; return I; }
  std::vector<uint32_t> chain(cf.begin(), cf.begin() + (nc > 0 ? coff[1] : 0));
  I.value = cv[0];
  I.before = (int)chain.size();
  if (getenv("ORACLE_DEBUG")) for (size_t i = 0; i < chain.size(); i++) fprintf(stderr, "  inner chain %zu: anchor %u q %u t %u len %d\n", i, chain[i], eq[chain[i]], et[chain[i]], el[chain[i]]);
  {                                                                   // RemovePairedIndels(ExtendBtwnPairs, BtwnChain, lengths)  Chain.h:753
    const int m = (int)chain.size();
    std::vector<uint32_t> cq(m), ct(m); std::vector<int> cln(m); std::vector<uint8_t> cs(m, 0), keep(std::max(m, 1)), lo(std::max(m, 1));
    for (int i = 0; i < m; i++) { cq[i] = eq[chain[i]]; ct[i] = et[chain[i]]; cln[i] = el[chain[i]]; }
    const int ops[1] = {5}; int nl = 0;
    oracle_filter_chain(m, cq.data(), ct.data(), cln.data(), cs.data(), nullptr, 0, ops, 1, keep.data(), lo.data(), &nl);
    std::vector<uint32_t> c2;
    for (int i = 0; i < m; i++) {
      if (keep[i]) { c2.push_back(chain[i]); if ((inversion || (long)chain[i] < ne - 2) && (I.keptMin < 0 || cln[i] < I.keptMin)) I.keptMin = cln[i]; }
      else I.rmMax = std::max(I.rmMax, cln[i]);
    }
    chain.swap(c2);
  }
  I.chain.swap(chain);
  if (I.chain.empty()) return I;
  I.be = (int)I.chain.size() - 1; I.bs = 0;
  if (I.chain.back() == (uint32_t)(ne - 1)) I.be = (int)I.chain.size() - 2;
  if (I.chain[0] == (uint32_t)(ne - 2)) I.bs = 1;
  uint32_t ce = curReadEnd, ge = curGenomeEnd;
  for (int btc = I.be; btc >= I.bs; btc--) { ce = eq[I.chain[btc]] + el[I.chain[btc]]; ge = et[I.chain[btc]] + el[I.chain[btc]]; }
  I.fin = nextGenomeStart > ge && nextReadStart > ce;
  I.np = (I.be >= I.bs ? I.be - I.bs + 1 : 0) + (I.fin ? 1 : 0);
  return I;
}

// RefinedAlignmentbtwnAnchors :203-550.  A = the chain's anchors (q, t, len) in chain order; alns.back() is the alignment being built.  tr: this pair's
// trace record or null.
void between_anchors(Env& E, int cur, int next, int str, int inv_str, int chrom, const uint32_t* AQ, const uint32_t* AT, const int* AL, std::vector<Aln>& alns,
                     bool& inversion, bool& breakalignment, double* tr) {
  Aln* alignment = &alns.back();
  const uint32_t L = E.readLen;
  if (str == 0) { alignment->blocks.push_back((int)AQ[cur]); alignment->blocks.push_back((int)AT[cur]); alignment->blocks.push_back(AL[cur]); }
  else { alignment->blocks.push_back((int)(L - AQ[cur] - AL[cur])); alignment->blocks.push_back((int)AT[cur]); alignment->blocks.push_back(AL[cur]); }
  uint32_t curGenomeEnd, curReadEnd, nextGenomeStart, nextReadStart;
  if (str == 0) { curReadEnd = AQ[cur] + AL[cur]; nextReadStart = AQ[next]; curGenomeEnd = AT[cur] + AL[cur]; nextGenomeStart = AT[next]; }
  else { curReadEnd = L - AQ[cur]; nextReadStart = L - AQ[next] - AL[next]; curGenomeEnd = AT[cur] + AL[cur]; nextGenomeStart = AT[next]; }
  if (tr) { tr[T_TYPE] = 0; tr[T_BLOCKS] = (double)(alns.back().blocks.size() / 3); }
  if (!(curGenomeEnd <= nextGenomeStart)) return;
  const long read_dist = (long)nextReadStart - (long)curReadEnd, genome_dist = (long)nextGenomeStart - (long)curGenomeEnd;   // (GenomePos differences widened to long)
  // note: nextReadStart - curReadEnd is unsigned arithmetic in the reference, converted to long: a "negative" distance is a huge value
  const long rd = (long)(uint32_t)(nextReadStart - curReadEnd), gd = (long)(uint32_t)(nextGenomeStart - curGenomeEnd);
  (void)read_dist; (void)genome_dist;
  if (tr) { tr[T_RD] = (double)rd; tr[T_GD] = (double)gd; }
  if (E.o->refineBySDP && std::min(rd, gd) >= 300) {
    int K, W, maxFreq = E.o->localMaxFreq;
    int refineSpaceDiag = 0;
    const int sv_diag = (int)(std::max(rd, gd) - std::min(rd, gd));
    if (!E.o->isOnt) refineSpaceDiag = std::min((int)std::floor(std::max(80.f, 0.01f * rd)), 500);
    else refineSpaceDiag = std::min((int)std::floor(std::max(100.f, 0.15f * rd)), 2000);
    refineSpaceDiag = std::max(2 * sv_diag, refineSpaceDiag);
    float minRatio;
    if (std::max(rd, gd) < 100) { K = 6; W = 5; minRatio = 0.5 / 29.5; }
    else if (std::max(rd, gd) < 500) { K = 9; W = 7; maxFreq = 50; minRatio = 0.5 / 69.1; }
    else { K = 12; W = 7; minRatio = 0.5 / 140.2; }
    if (tr) { tr[T_TYPE] = 2; tr[T_K] = K; tr[T_W] = W; tr[T_MF] = maxFreq; tr[T_DIAG] = refineSpaceDiag; tr[T_SV] = sv_diag; }
    std::vector<uint32_t> fq, ft, rq, rt;
    float identity = 0;
    refine_space(E, K, W, refineSpaceDiag, maxFreq, chrom, nextReadStart, curReadEnd, nextGenomeStart, curGenomeEnd, str, fq, ft, identity);
    if (E.bad) return;
    const int minDist = (int)std::min(rd, gd);
    bool useRev = false;
    if (getenv("ORACLE_DEBUG")) fprintf(stderr, "big space: rd %ld gd %ld K %d nF %zu id %f minRatio %f blocks %zu\n", rd, gd, K, fq.size(), identity, minRatio, alns.back().blocks.size() / 3);
    if (tr) {                                                             // the device's plan for this space (see the enum)
      const bool super = (fq.size() / (float)minDist) < minRatio && identity < 0.8;
      tr[T_NF] = (double)fq.size(); tr[T_IDF] = identity; tr[T_SUPER] = super; tr[T_TRIED] = 0;
      int jobs = fq.size() > 0, np2 = 0, spec = 1;
      if (fq.size() > 0) np2 += plan_inner(E, fq, ft, false, K, chrom, curReadEnd, curGenomeEnd, nextReadStart, nextGenomeStart, AL[cur], AL[next]).np; else np2 += 1;
      if (super) {
        Env E2 = E;
        std::vector<uint32_t> sq2, st2; float id2 = 0;
        const uint32_t cre2 = L - nextReadStart, nrs2 = L - curReadEnd;
        refine_space(E2, K, E.o->globalW, refineSpaceDiag, maxFreq, chrom, nrs2, cre2, nextGenomeStart, curGenomeEnd, inv_str, sq2, st2, id2);
        if (!E2.bad) {
          spec = decide(E.o, fq.size(), sq2.size(), id2, minDist, sv_diag, minRatio);
          if (spec == 2) { jobs++; np2 += plan_inner(E, sq2, st2, true, K, chrom, cre2, curGenomeEnd, nrs2, nextGenomeStart, AL[cur], AL[next]).np; }
        }
      }
      tr[T_SPEC] = spec; tr[T_JOBS] = jobs; tr[T_NP2] = np2;
    }
    if ((fq.size() / (float)minDist) < minRatio && alns.back().blocks.size() / 3 >= 5 && identity < 0.8) {   // try the other strand
      const uint32_t temp = curReadEnd;
      curReadEnd = L - nextReadStart; nextReadStart = L - temp;
      identity = 0;
      refine_space(E, K, E.o->globalW, refineSpaceDiag, maxFreq, chrom, nextReadStart, curReadEnd, nextGenomeStart, curGenomeEnd, inv_str, rq, rt, identity);
      if (E.bad) return;
      if (tr) { tr[T_TRIED] = 1; tr[T_NR] = (double)rq.size(); tr[T_IDR] = identity; }
      const int oc = decide(E.o, fq.size(), rq.size(), identity, minDist, sv_diag, minRatio);
      if (oc == 0) { breakalignment = 1; inversion = 0; if (tr) tr[T_OUTCOME] = 0; return; }
      if (oc == 1) {
        inversion = 0;
        const uint32_t t2 = curReadEnd;
        curReadEnd = L - nextReadStart; nextReadStart = L - t2;
      } else { useRev = true; inversion = 1; }
    }
    std::vector<uint32_t>& bq = useRev ? rq : fq;
    std::vector<uint32_t>& bt = useRev ? rt : ft;
    if (tr) tr[T_OUTCOME] = bq.size() > 0 ? (useRev ? 2 : 1) : 3;
    if (bq.size() > 0) {
      const Inner I = plan_inner(E, bq, bt, inversion, K, chrom, curReadEnd, curGenomeEnd, nextReadStart, nextGenomeStart, AL[cur], AL[next]);
      if (I.sdpBad) { E.bad = true; return; }
      if (tr) { tr[T_IN_BEFORE] = I.before; tr[T_IN_AFTER] = (double)I.chain.size(); tr[T_RM_MAX] = I.rmMax; tr[T_KEPT_MIN] = I.keptMin; }
      if (I.chain.empty()) { E.bad = true; return; }                      // BtwnChain.back() on an empty vector
      const std::vector<uint32_t>& chain = I.chain; const std::vector<uint32_t>& eq = I.eq; const std::vector<uint32_t>& et = I.et; const std::vector<int>& el = I.el;
      uint32_t btc_curReadEnd = curReadEnd, btc_curGenomeEnd = curGenomeEnd;
      const int btc_end = I.be, btc_start = I.bs;
      if (tr) { tr[T_BTC_START] = btc_start; tr[T_BTC_END] = btc_end; tr[T_FINAL] = I.fin; }
      if (inversion == 1) {
        Aln inv; inv.strand = inv_str; inv.supp = 1; inv.secondary = 0; inv.N0 = (int)chain.size(); inv.N1 = (int)chain.size(); inv.chrom = chrom; inv.value = I.value;
        alns.push_back(inv);
      }
      for (int btc = btc_end; btc >= btc_start; btc--) {
        const uint32_t ngs = et[chain[btc]], nrs = eq[chain[btc]];
        linear_between(E, btc_curReadEnd, btc_curGenomeEnd, nrs, ngs, str, chrom, &alns.back());
        if (E.bad) return;
        alns.back().blocks.push_back((int)nrs); alns.back().blocks.push_back((int)ngs); alns.back().blocks.push_back(el[chain[btc]]);
        btc_curReadEnd = nrs + el[chain[btc]]; btc_curGenomeEnd = ngs + el[chain[btc]];
      }
      if (nextGenomeStart > btc_curGenomeEnd && nextReadStart > btc_curReadEnd) linear_between(E, btc_curReadEnd, btc_curGenomeEnd, nextReadStart, nextGenomeStart, str, chrom, &alns.back());
    } else linear_between(E, curReadEnd, curGenomeEnd, nextReadStart, nextGenomeStart, str, chrom, &alns.back());
  } else { if (tr) tr[T_TYPE] = 1; linear_between(E, curReadEnd, curGenomeEnd, nextReadStart, nextGenomeStart, str, chrom, &alns.back()); }
}

}  // namespace

// One primary chain h of one read: nChains chains (the second sparse DP's, after its filters) as CSR over anchors (q, t chromosome-relative,
// len), per chain strand / chromIndex / FirstSDPValue / NumOfAnchors0 / NumOfAnchors1; LSC = LargestSplitChain.  Out: the SegAlignments pushed
// onto alignments.back() in order: strand, Supplymentary, ISsecondary, NumOfAnchors0/1, value, chromIndex and blocks (CSR of qPos, tPos,
// length).  Returns the number of alignments, -1 when the reference would read outside an array, -2 when a capacity is too small.
extern "C" int oracle_local_refine_alignment_ex(int nChains, const int* chainOff, const uint32_t* aq, const uint32_t* at, const int* alen, const uint8_t* chainStrand,
                                                const int* chainChrom, const float* firstSdp, const int* numAnchors0, const int* numAnchors1, int LSC, int h, int minAnchors,
                                                const char* fwd, const char* rc, uint32_t readLen, const char* genome, const uint64_t* chromPos, const oracle_lra_opts* o,
                                                int maxSeg, int* segStrand, int* segSupp, int* segSecondary, int* segN0, int* segN1, float* segValue, int* segChrom,
                                                int* segBlockOff, int* blocks, long blockCap);
extern "C" int oracle_local_refine_alignment(int nChains, const int* chainOff, const uint32_t* aq, const uint32_t* at, const int* alen, const uint8_t* chainStrand,
                                             const int* chainChrom, const float* firstSdp, const int* numAnchors0, const int* numAnchors1, int LSC, int h,
                                             const char* fwd, const char* rc, uint32_t readLen, const char* genome, const uint64_t* chromPos, const oracle_lra_opts* o,
                                             int maxSeg, int* segStrand, int* segSupp, int* segSecondary, int* segN0, int* segN1, float* segValue, int* segChrom,
                                             int* segBlockOff, int* blocks, long blockCap) {
  return oracle_local_refine_alignment_ex(nChains, chainOff, aq, at, alen, chainStrand, chainChrom, firstSdp, numAnchors0, numAnchors1, LSC, h, 2, fwd, rc, readLen, genome,
                                          chromPos, o, maxSeg, segStrand, segSupp, segSecondary, segN0, segN1, segValue, segChrom, segBlockOff, blocks, blockCap);
}
// minAnchors = 1: the walk of the high-accuracy overload (LocalRefineAlignment.h:577-766; `if (ultimatechain.size() == 0) continue`, :579), whose chains st are
// splitchains[st] (empty where the ultimatechain is empty), LSC = LargestSplitChain_dist, firstSdp / numAnchors0 = chains[h].value / NumOfAnchors0.
extern "C" int oracle_lr_trace_fields() { return T_N; }
// the same with a trace: up to traceCap records of oracle_lr_trace_fields() doubles, one per anchor pair in walk order, *nTrace of them written (also when the
// result is -1: the pairs walked so far).  trace = null: nothing else changes.
extern "C" int oracle_local_refine_alignment_trace(int nChains, const int* chainOff, const uint32_t* aq, const uint32_t* at, const int* alen, const uint8_t* chainStrand,
                                                   const int* chainChrom, const float* firstSdp, const int* numAnchors0, const int* numAnchors1, int LSC, int h, int minAnchors,
                                                   const char* fwd, const char* rc, uint32_t readLen, const char* genome, const uint64_t* chromPos, const oracle_lra_opts* o,
                                                   int maxSeg, int* segStrand, int* segSupp, int* segSecondary, int* segN0, int* segN1, float* segValue, int* segChrom,
                                                   int* segBlockOff, int* blocks, long blockCap, double* trace, int traceCap, int* nTrace);
extern "C" int oracle_local_refine_alignment_ex(int nChains, const int* chainOff, const uint32_t* aq, const uint32_t* at, const int* alen, const uint8_t* chainStrand,
                                                const int* chainChrom, const float* firstSdp, const int* numAnchors0, const int* numAnchors1, int LSC, int h, int minAnchors,
                                                const char* fwd, const char* rc, uint32_t readLen, const char* genome, const uint64_t* chromPos, const oracle_lra_opts* o,
                                                int maxSeg, int* segStrand, int* segSupp, int* segSecondary, int* segN0, int* segN1, float* segValue, int* segChrom,
                                                int* segBlockOff, int* blocks, long blockCap) {
  return oracle_local_refine_alignment_trace(nChains, chainOff, aq, at, alen, chainStrand, chainChrom, firstSdp, numAnchors0, numAnchors1, LSC, h, minAnchors, fwd, rc, readLen,
                                             genome, chromPos, o, maxSeg, segStrand, segSupp, segSecondary, segN0, segN1, segValue, segChrom, segBlockOff, blocks, blockCap,
                                             nullptr, 0, nullptr);
}
extern "C" int oracle_local_refine_alignment_trace(int nChains, const int* chainOff, const uint32_t* aq, const uint32_t* at, const int* alen, const uint8_t* chainStrand,
                                                   const int* chainChrom, const float* firstSdp, const int* numAnchors0, const int* numAnchors1, int LSC, int h, int minAnchors,
                                                   const char* fwd, const char* rc, uint32_t readLen, const char* genome, const uint64_t* chromPos, const oracle_lra_opts* o,
                                                   int maxSeg, int* segStrand, int* segSupp, int* segSecondary, int* segN0, int* segN1, float* segValue, int* segChrom,
                                                   int* segBlockOff, int* blocks, long blockCap, double* trace, int traceCap, int* nTrace) {
  if (nTrace) *nTrace = 0;
  auto record = [&](int st, int cur) -> double* {
    if (!trace || !nTrace || *nTrace >= traceCap) return nullptr;
    double* tr = trace + (size_t)T_N * (*nTrace)++;
    for (int i = 0; i < T_N; i++) tr[i] = -1;
    tr[T_CHAIN] = st; tr[T_CUR] = cur;
    return tr;
  };
  Env E; E.strands[0] = fwd; E.strands[1] = rc; E.readLen = readLen; E.genome = genome; E.chromPos = chromPos; E.o = o;
  std::vector<Aln> alns;
  for (int st = 0; st < nChains; st++) {
    const int m = chainOff[st + 1] - chainOff[st];
    if (m < minAnchors) continue;
    const uint32_t* AQ = aq + chainOff[st]; const uint32_t* AT = at + chainOff[st]; const int* AL = alen + chainOff[st];
    const int start = 0, end = m - 1;
    const int str = chainStrand[st], chrom = chainChrom[st];
    auto fresh = [&](int supp) { Aln a; a.strand = str; a.supp = supp; a.secondary = 0; a.N0 = numAnchors0[st]; a.N1 = 0; a.chrom = chrom; a.value = firstSdp[st]; return a; };
    Aln first = fresh(0);
    first.N1 = numAnchors1[st];
    if (h > 0) first.secondary = 1;
    if (st != LSC) first.supp = 1;
    alns.push_back(first);
    bool inversion = 0, breakalignment = 0;
    auto on_event = [&](int inv_str, int n1) {
      alns.back().strand = inversion ? inv_str : str;                     // UpdateParameters(inv_str / str, ...) :506-511
      alns.back().N0 = numAnchors0[st]; alns.back().N1 = n1;
      alns.push_back(fresh(1));
      inversion = 0; breakalignment = 0;
    };
    if (str == 0) {
      int last = end, fl = end;
      const int inv_str = 1;
      while (fl > start) {
        between_anchors(E, fl, fl - 1, str, inv_str, chrom, AQ, AT, AL, alns, inversion, breakalignment, record(st, fl));
        if (E.bad) return -1;
        if (inversion || breakalignment) { on_event(inv_str, last - fl); last = fl; }
        fl--;
      }
      alns.back().N0 = numAnchors0[st]; alns.back().N1 = last - fl;
      alns.back().blocks.push_back((int)AQ[start]); alns.back().blocks.push_back((int)AT[start]); alns.back().blocks.push_back(AL[start]);
    } else {
      int last = start, fl = start;
      const int inv_str = 0;
      while (fl < end) {
        between_anchors(E, fl, fl + 1, str, inv_str, chrom, AQ, AT, AL, alns, inversion, breakalignment, record(st, fl));
        if (E.bad) return -1;
        if (inversion || breakalignment) { on_event(inv_str, fl - last); last = fl; }
        fl++;
      }
      alns.back().N0 = numAnchors0[st]; alns.back().N1 = fl - last;
      alns.back().blocks.push_back((int)(readLen - AQ[end] - AL[end])); alns.back().blocks.push_back((int)AT[end]); alns.back().blocks.push_back(AL[end]);
    }
    alns.back().strand = str;                                             // UpdateParameters(str, ...) :995
  }
  if ((int)alns.size() > maxSeg) return -2;
  long nb = 0;
  segBlockOff[0] = 0;
  for (size_t i = 0; i < alns.size(); i++) {
    segStrand[i] = alns[i].strand; segSupp[i] = alns[i].supp; segSecondary[i] = alns[i].secondary; segN0[i] = alns[i].N0; segN1[i] = alns[i].N1;
    segValue[i] = alns[i].value; segChrom[i] = alns[i].chrom;
    if (nb + (long)alns[i].blocks.size() / 3 > blockCap) return -2;
    for (size_t k = 0; k < alns[i].blocks.size(); k++) blocks[3 * nb + k] = alns[i].blocks[k];
    nb += (long)alns[i].blocks.size() / 3;
    segBlockOff[i + 1] = (int)nb;
  }
  return (int)alns.size();
}

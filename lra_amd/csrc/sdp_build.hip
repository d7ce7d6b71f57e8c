// lra_amd/csrc/sdp_build.hip -- the sparse DP's decompositions (sdp.h lists the files; the design is described in sdp.hip): sdp_build, the count pass and the emit pass
// of the four divide-and-conquer trees of every read, a wave per read or a 1024-thread workgroup per large read.  gfx950 only.
// The visit records (sub-problem id, index in Di / Ei of a point on a level) go to the read's visit PLANES (sdp.h, ReadArena): pass F of a level writes the one plane of
// its (family pair, level), vis[plane * P + point] -- one contiguous 8 P bytes within the level instead of one 8-byte slot in every point's own row -- and never a level the
// read has no plane for: that read is given up with LRA_ST_RANGE, as one beyond LV levels is.
#include "sdp.h"
#include <type_traits>

using namespace lra_sdp;

namespace {

// NW = waves per read: 1 (a wave per read) or 16 (a 1024-thread workgroup per LARGE read: every pass over the read's points is spread over the block, the
// wave scans become block scans through LDS; the same arithmetic, the same tables).
template <int NW>
__device__ __forceinline__ int blk_incl_scan(int v, int lane, int wave, int* s_w, int& total) {
  const int inc = wave_incl_scan(v, lane);
  if (NW == 1) { total = __builtin_amdgcn_readlane(inc, 63); return inc; }
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  int pre = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NW; w++) { const int x = s_w[w]; tot += x; if (w < wave) pre += x; }
  __syncthreads();
  total = tot;
  return inc + pre;
}
// LDSV (one wave per read, at most 512 points): the per-element arrays -- 28 bytes per point with 16-bit indices and 32-bit diagonals -- live in the wave's LDS.
// From the scratch arena every level streams them through HBM again (2.6 KB per point and build: 250 GB per step, a third of the step's traffic).
// MODE 2: the same narrow arrays in the arena (reads of 513 .. 16383 points: half the bytes per level, no LDS to run out of).  MODE 0: 32-bit indices, 64-bit diagonals.
// BSTAT (LRA_SDP_BUILD_STAT): cycles per pass -- an instantiation of its own: the kernel spills as it is, and the counter's two scalars more than double what it spills
template <bool EMIT, int NW, int MODE = 0, int OCC = 8, bool BSTAT = false>
__global__ void __launch_bounds__(64 * NW, NW == 1 ? OCC : 1) sdp_build(BuildArgs a) {
  constexpr int NT = 64 * NW;
  constexpr bool LDSV = MODE == 1, NARROW = MODE != 0;
  using IT = typename std::conditional<NARROW, uint16_t, uint32_t>::type; // element -> node / position / line / prefix count
  using DT = typename std::conditional<NARROW, uint32_t, long long>::type; // a diagonal (compared for equality only: 32 bits of it identify it inside one read)
  constexpr IT INONE = (IT)~(IT)0;
  extern __shared__ __attribute__((aligned(16))) char dyn_lds[];
  __shared__ int s_w[4][NW == 1 ? 1 : NW];
  __shared__ unsigned long long s_bt[BSTAT ? 8 : 1];
  unsigned long long btPrev = 0;
  constexpr bool bstat = BSTAT;
  if (bstat) { if (threadIdx.x < 8) s_bt[threadIdx.x] = 0; btPrev = __builtin_amdgcn_s_memtime(); }
#define BTICK(k_) do { if (bstat) { const unsigned long long t__ = __builtin_amdgcn_s_memtime(); if (threadIdx.x == 0) s_bt[k_] += t__ - btPrev; btPrev = t__; } } while (0)
  const int rr = (int)a.order[blockIdx.x], r = a.r0 + rr, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  auto SYNC = [&]() { if (NW == 1) wave_sync(); else __syncthreads(); };
  const uint64_t p0 = a.ptOff[r], pc0 = a.ptOff[a.r0];
  const int P = (int)(a.ptOff[r + 1] - p0);
  if (P == 0) { if (tid == 0) { if (!EMIT) { a.cntEntries[rr] = 0; a.cntNodes[rr] = 0; a.cntD[rr] = 0; } a.cntV[rr] = 0; a.cntRC[rr] = 0; } return; }
  const uint32_t* hq = a.hq + p0; const uint32_t* ht = a.ht + p0; const uint32_t* h2 = a.h2 + p0;
  const uint64_t* key3 = a.key3 + p0; const uint32_t* pay3 = a.pay3 + p0;
  uint32_t* S = a.scratch + 34 * (p0 - pc0) + 64 * (uint64_t)rr;
  const int NCAP = P + 2;
  // the arena's layout (34 words per point); LDSV uses its node tables only
  uint32_t* tbl = S + 8 * P + 2;            // [2][6][NCAP]
  uint32_t* tmp = tbl + 12 * NCAP;          // [8][NCAP]
  IT* eb_ = LDSV ? (IT*)dyn_lds : (IT*)S;
  IT* rowOf = eb_; IT* colOf = rowOf + P;
  IT* lp = colOf + P;                       // [2][P]
  IT* ln = lp + 2 * P;                      // [2][P]: [0] node index of the element, [1] temporary 2k+side
  IT* pf = ln + 2 * P;                      // [P+1]
  IT* ph = pf + P + 1;                      // [P+1]
  // MODE 0: ll and ld behind the tables (word offset 30 P + 42 from S: even, so ld is 8-byte aligned); narrow: ll behind ph, ld behind the tables / behind ll in LDS
  IT* ll = NARROW ? ph + P + 1 : (IT*)(tmp + 8 * NCAP);   // [2][P]  line (row / column index) of the element: travels with it, no gathers per level
  DT* ld = LDSV ? (DT*)(dyn_lds + ((((size_t)(10 * P + 2) * sizeof(IT)) + 7) & ~(size_t)7)) : NARROW ? (DT*)(tmp + 8 * NCAP) : (DT*)(ll + 2 * P);   // [2][P]  its diagonal
  auto LN = [&](int idx) -> uint32_t { const IT v = ln[idx]; return v == INONE ? NONE : (uint32_t)v; };
#define TB(c, f, k) tbl[((c) * 6 + (f)) * NCAP + (k)]
#define TM(f, k) tmp[(f) * NCAP + (k)]
  enum { F_LS, F_LE, F_SB, F_SE, F_EB, F_EE };
  enum { T_C1S, T_C1E, T_ND, T_NE, T_CH0, T_CH1, T_BASE, T_GID };
  // rows (GetRowInfo) and columns (GetColInfo): index of the distinct q / t of every point
  int R = 0, C = 0;
  for (int i0 = 0; i0 < P; i0 += NT) {
    const int i = i0 + tid;
    const int head = (i < P) && (i == 0 || hq[i] != hq[i - 1]);
    int tot; const int inc = blk_incl_scan<NW>(head, lane, wave, s_w[0], tot);
    if (i < P) rowOf[i] = R + inc - 1;
    R += tot;
  }
  for (int i0 = 0; i0 < P; i0 += NT) {
    const int i = i0 + tid;
    const int head = (i < P) && (i == 0 || ht[h2[i]] != ht[h2[i - 1]]);
    int tot; const int inc = blk_incl_scan<NW>(head, lane, wave, s_w[0], tot);
    if (i < P) colOf[h2[i]] = C + inc - 1;
    C += tot;
  }
  // class boundaries in the diagonal-sorted list
  int cOff[5];
  {
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int i = tid; i < P; i += NT) { const int cl = (int)(key3[i] >> 40); c0 += cl == 0; c1 += cl == 1; c2 += cl == 2; c3 += cl == 3; }
    for (int o = 32; o > 0; o >>= 1) { c0 += __shfl_xor(c0, o); c1 += __shfl_xor(c1, o); c2 += __shfl_xor(c2, o); c3 += __shfl_xor(c3, o); }
    if (NW > 1) {
      if (lane == 0) { s_w[0][wave] = c0; s_w[1][wave] = c1; s_w[2][wave] = c2; s_w[3][wave] = c3; }
      __syncthreads();
      c0 = c1 = c2 = c3 = 0;
      for (int w = 0; w < NW; w++) { c0 += s_w[0][w]; c1 += s_w[1][w]; c2 += s_w[2][w]; c3 += s_w[3][w]; }
      __syncthreads();
    }
    // (the same number in every lane, but made by shuffles: said to be uniform, the class boundaries live in scalar registers -- as vector registers they are live through the
    // whole kernel and are what the register allocator spills to scratch, to be read back inside every level)
    c0 = __builtin_amdgcn_readfirstlane(c0); c1 = __builtin_amdgcn_readfirstlane(c1); c2 = __builtin_amdgcn_readfirstlane(c2);
    cOff[0] = 0; cOff[1] = c0; cOff[2] = c0 + c1; cOff[3] = c0 + c1 + c2; cOff[4] = P;
  }
  SYNC();
  BTICK(0);
  uint32_t nEntries = 0, nNodesTot = 0, sumD = 0, nVisits = 0;
  Node* nodesR = nullptr; Ent* entR = nullptr; uint32_t* apR = nullptr; int2* stkR = nullptr; uint2* visR = nullptr; long long* edR = nullptr;
  uint32_t blkPair = 0, visPl = 0;
  if (EMIT) {
    const ReadArena A = a.ra[rr];
    char* b = arena_ptr(A.base);
    blkPair = A.blkPair; visPl = A.visPl;
    nodesR = (Node*)b; entR = (Ent*)(b + A.entOff); apR = (uint32_t*)(b + A.apOff); stkR = (int2*)(b + A.stkOff); visR = (uint2*)(b + A.visOff);
    edR = (long long*)(b + A.edOff);
  }
  bool overflow = false, outgrown = false;
  const uint64_t capE = EMIT ? a.cntEntries[rr] : 0, capN = EMIT ? a.cntNodes[rr] : 0, capD = EMIT ? a.cntD[rr] : 0;
  for (int fam = 0; fam < 4 && !outgrown; fam++) {
    // family switches (DivideSubBy{Row1,Col1,Row2,Col2}.h): R1, C1, R2, C2
    const bool col = fam & 1, back = fam >= 2, desc = (fam == 1 || fam == 2), swapped = (fam == 3);
    const IT* lineOf = col ? colOf : rowOf;
    const int nLines = col ? C : R;
    const int sc = back ? 2 : 0;
    const int nS = cOff[sc + 1] - cOff[sc], nEn = cOff[sc + 2] - cOff[sc + 1], Pf = nS + nEn;
    if (nS == 0 || nEn == 0) continue;
    const int fam2 = fam & 1;
    // the family pair's visit planes: one per level the read was laid out for (ReadArena::visPl), the column family's behind the row family's
    const int nPl = EMIT ? (int)(fam2 ? visPl >> 8 : visPl & 0xffu) : LV;
    uint2* visF = EMIT ? visR + (size_t)(fam2 ? visPl & 0xffu : 0u) * P : nullptr;
    const int dSide = swapped ? 1 : 0, eSide = swapped ? 0 : 1;
    for (int i = tid; i < Pf; i += NT) {
      const uint32_t pos = pay3[cOff[sc] + i];
      lp[i] = (IT)pos; ln[i] = 0; ll[i] = lineOf[pos];
      ld[i] = (DT)(back ? (long long)ht[pos] + hq[pos] : (long long)ht[pos] - hq[pos]);
    }
    if (tid == 0) { TB(0, F_LS, 0) = 0; TB(0, F_LE, 0) = nLines; TB(0, F_SB, 0) = 0; TB(0, F_SE, 0) = nS; TB(0, F_EB, 0) = nS; TB(0, F_EE, 0) = Pf; }
    int nNodes = 1, cur = 0;
    SYNC();
    BTICK(7);
    for (int level = 0; nNodes > 0 && !outgrown; level++) {
      if (level >= nPl) { overflow = true; break; }                        // (a level without a plane is never written.  Laid out from the read's rows / columns
                                                                            // or from its points, the planes fall short only beyond LV levels)
      uint2* visL = EMIT ? visF + (size_t)level * P : nullptr;
      const int nxt = cur ^ 1;
      IT* lpc = lp + cur * P; IT* lpn = lp + nxt * P;
      IT* llc = ll + cur * P; IT* lln = ll + nxt * P;
      DT* ldc = ld + (size_t)cur * P; DT* ldn = ld + (size_t)nxt * P;
      // A: which elements go to the first half of their node's lines; exclusive prefix in pf
      {
        int carry = 0;
        // (UA chunks of the pass at a time: their loads -- node of the element, the node's line range, the element's line -- are all asked for before anything is
        // waited for or stored, so a chunk costs a third of a dependent chain instead of a whole one; the pass is a latency chain per wave, not a stream)
        constexpr int UA = 4;
        for (int i0 = 0; i0 < Pf; i0 += UA * NT) {
          uint32_t kk[UA]; uint32_t ss[UA], ee[UA]; IT lv[UA]; int ff[UA];
#pragma unroll
          for (int u = 0; u < UA; u++) { const int i = i0 + u * NT + tid; kk[u] = i < Pf ? LN(i) : NONE; lv[u] = i < Pf ? llc[i] : (IT)0; }
#pragma unroll
          for (int u = 0; u < UA; u++) { ss[u] = 0; ee[u] = 0; if (kk[u] != NONE) { ss[u] = TB(cur, F_LS, kk[u]); ee[u] = TB(cur, F_LE, kk[u]); } }
#pragma unroll
          for (int u = 0; u < UA; u++) ff[u] = kk[u] == NONE ? 0 : (ee[u] - ss[u] > 1) ? (lv[u] < ((ss[u] + ee[u]) >> 1)) : 1;
#pragma unroll
          for (int u = 0; u < UA; u++) {
            const int i = i0 + u * NT + tid;
            if (i0 + u * NT >= Pf) break;
            int tot; const int inc = blk_incl_scan<NW>(ff[u], lane, wave, s_w[0], tot);
            if (i < Pf) pf[i] = (IT)(carry + inc - ff[u]);
            carry += tot;
          }
        }
        if (tid == 0) pf[Pf] = (IT)carry;
      }
      SYNC();
      BTICK(1);
      for (int k = tid; k < nNodes; k += NT) {
        TM(T_C1S, k) = (uint32_t)pf[TB(cur, F_SE, k)] - (uint32_t)pf[TB(cur, F_SB, k)];
        TM(T_C1E, k) = (uint32_t)pf[TB(cur, F_EE, k)] - (uint32_t)pf[TB(cur, F_EB, k)];
      }
      SYNC();
      // C: stable partition of every node's two segments
      {
        // (a node's two segments are partitioned inside their own ranges, so an element's slot ln[P + .] is written either here (no node) or by the element that moves
        // into it, never both: the chunks of a group may be read before any of them is written)
        constexpr int UC = 2;
        for (int i0 = 0; i0 < Pf; i0 += UC * NT) {
          uint32_t kk[UC], pi0[UC], pi1[UC], sb[UC], c1[UC], psb[UC]; IT vlp[UC], vll[UC]; DT vld[UC];
#pragma unroll
          for (int u = 0; u < UC; u++) {
            const int i = i0 + u * NT + tid;
            kk[u] = NONE; pi0[u] = 0; pi1[u] = 0; vlp[u] = 0; vll[u] = 0; vld[u] = 0;
            if (i < Pf) { kk[u] = LN(i); pi0[u] = (uint32_t)pf[i]; pi1[u] = (uint32_t)pf[i + 1]; vlp[u] = lpc[i]; vll[u] = llc[i]; vld[u] = ldc[i]; }
          }
#pragma unroll
          for (int u = 0; u < UC; u++) {
            const int i = i0 + u * NT + tid;
            const bool isS = i < nS;
            sb[u] = 0; c1[u] = 0;
            if (kk[u] != NONE) { sb[u] = isS ? TB(cur, F_SB, kk[u]) : TB(cur, F_EB, kk[u]); c1[u] = isS ? TM(T_C1S, kk[u]) : TM(T_C1E, kk[u]); }
          }
#pragma unroll
          for (int u = 0; u < UC; u++) psb[u] = kk[u] != NONE ? (uint32_t)pf[sb[u]] : 0;
#pragma unroll
          for (int u = 0; u < UC; u++) {
            const int i = i0 + u * NT + tid;
            if (i >= Pf) continue;
            if (kk[u] == NONE) { ln[P + i] = INONE; continue; }
            const uint32_t rank1 = pi0[u] - psb[u];
            const uint32_t first = pi1[u] - pi0[u];
            const uint32_t np_ = first ? sb[u] + rank1 : sb[u] + c1[u] + ((uint32_t)i - sb[u] - rank1);
            lpn[np_] = vlp[u]; lln[np_] = vll[u]; ldn[np_] = vld[u];
            ln[P + np_] = (IT)(2 * kk[u] + (first ? 0 : 1));
          }
        }
      }
      SYNC();
      BTICK(2);
      // D: heads of the distinct diagonals inside the D segment (ends) / E segment (starts); exclusive prefix in ph
      {
        int carry = 0;
        constexpr int UD = NW == 1 ? 4 : 2;
        for (int j0 = 0; j0 < Pf; j0 += UD * NT) {
          uint32_t k2v[UD], le[UD], ls[UD], bg[UD], c1[UD]; DT d0[UD], d1[UD]; int hd[UD];
#pragma unroll
          for (int u = 0; u < UD; u++) {
            const int j = j0 + u * NT + tid;
            k2v[u] = NONE; d0[u] = 0; d1[u] = 0;
            if (j < Pf) { k2v[u] = LN(P + j); d0[u] = ldn[j]; d1[u] = j > 0 ? ldn[j - 1] : ldn[j]; }
          }
#pragma unroll
          for (int u = 0; u < UD; u++) {
            const int j = j0 + u * NT + tid;
            const bool isS = j < nS;
            le[u] = 0; ls[u] = 0; bg[u] = 0; c1[u] = 0;
            if (k2v[u] != NONE) {
              const uint32_t k = k2v[u] >> 1;
              le[u] = TB(cur, F_LE, k); ls[u] = TB(cur, F_LS, k); bg[u] = isS ? TB(cur, F_SB, k) : TB(cur, F_EB, k); c1[u] = isS ? TM(T_C1S, k) : TM(T_C1E, k);
            }
          }
#pragma unroll
          for (int u = 0; u < UD; u++) {
            const int j = j0 + u * NT + tid;
            hd[u] = 0;
            if (k2v[u] != NONE) {
              const uint32_t side = k2v[u] & 1;
              const bool isS = j < nS;
              const bool leaf = le[u] - ls[u] == 1;
              const bool in = leaf || (int)side == (isS ? eSide : dSide);
              if (in) {
                uint32_t beg = bg[u];
                if (!leaf && side == 1) beg += c1[u];
                hd[u] = ((uint32_t)j == beg) ? 1 : (d0[u] != d1[u]);
              }
            }
          }
#pragma unroll
          for (int u = 0; u < UD; u++) {
            const int j = j0 + u * NT + tid;
            if (j0 + u * NT >= Pf) break;
            int tot; const int inc = blk_incl_scan<NW>(hd[u], lane, wave, s_w[0], tot);
            if (j < Pf) ph[j] = (IT)(carry + inc - hd[u]);
            carry += tot;
          }
        }
        if (tid == 0) ph[Pf] = (IT)carry;
      }
      SYNC();
      BTICK(3);
      // E: per node: sizes, fullness, children, next level's table
      int nNext = 0;
      for (int k0 = 0; k0 < nNodes; k0 += NT) {
        const int k = k0 + tid;
        uint32_t nD = 0, nE = 0, act0 = 0, act1 = 0, full = 0;
        uint32_t ls = 0, le = 0, sb = 0, se = 0, eb = 0, ee = 0, c1S = 0, c1E = 0;
        bool leaf = false;
        if (k < nNodes) {
          ls = TB(cur, F_LS, k); le = TB(cur, F_LE, k); sb = TB(cur, F_SB, k); se = TB(cur, F_SE, k); eb = TB(cur, F_EB, k); ee = TB(cur, F_EE, k);
          c1S = TM(T_C1S, k); c1E = TM(T_C1E, k);
          leaf = le - ls == 1;
          uint32_t dB, dE, eB, eE;
          if (leaf) { dB = eb; dE = ee; eB = sb; eE = se; }
          else {
            dB = dSide == 0 ? eb : eb + c1E; dE = dSide == 0 ? eb + c1E : ee;
            eB = eSide == 0 ? sb : sb + c1S; eE = eSide == 0 ? sb + c1S : se;
          }
          nD = (uint32_t)ph[dE] - (uint32_t)ph[dB]; nE = (uint32_t)ph[eE] - (uint32_t)ph[eB];
          full = nD > 0 && nE > 0;
          if (!leaf) {                                                   // DivideSubProbBy*: which halves are explored
            const bool goD = nD > 0, goE = nE > 0;                       // both empty: none; only Di: D half; only Ei: E half; else both
            if (dSide == 0) { act0 = goD; act1 = goE; } else { act1 = goD; act0 = goE; }
          }
        }
        int totF, totEnt, totD, totC;
        const int incF = blk_incl_scan<NW>((int)full, lane, wave, s_w[0], totF), incEnt = blk_incl_scan<NW>((int)(full ? nD + nE : 0), lane, wave, s_w[1], totEnt),
                  incD = blk_incl_scan<NW>((int)(full ? nD : 0), lane, wave, s_w[2], totD), incC = blk_incl_scan<NW>((int)(act0 + act1), lane, wave, s_w[3], totC);
        // the read's blocks may have been laid out from an estimate (k_arena_estimate): nothing is written past them -- the level is abandoned (the levels before it are
        // complete, and nothing points at this one yet) and the read is built again from exact counts
        if (EMIT && ((uint64_t)nNodesTot + totF > capN || (uint64_t)nEntries + totEnt > capE || (uint64_t)sumD + totD > capD)) { outgrown = true; break; }
        if (k < nNodes) {
          const uint32_t gid = nNodesTot + incF - full, base = nEntries + incEnt - (full ? nD + nE : 0), dpre = sumD + incD - (full ? nD : 0);
          TM(T_ND, k) = nD; TM(T_NE, k) = nE; TM(T_GID, k) = full ? gid : NONE; TM(T_BASE, k) = base;
          uint32_t ci = nNext + incC - (act0 + act1);
          const uint32_t med = (ls + le) >> 1;
          TM(T_CH0, k) = NONE; TM(T_CH1, k) = NONE;
          if (act0) { TM(T_CH0, k) = ci; TB(nxt, F_LS, ci) = ls; TB(nxt, F_LE, ci) = med; TB(nxt, F_SB, ci) = sb; TB(nxt, F_SE, ci) = sb + c1S;
                      TB(nxt, F_EB, ci) = eb; TB(nxt, F_EE, ci) = eb + c1E; ci++; }
          if (act1) { TM(T_CH1, k) = ci; TB(nxt, F_LS, ci) = med; TB(nxt, F_LE, ci) = le; TB(nxt, F_SB, ci) = sb + c1S; TB(nxt, F_SE, ci) = se;
                      TB(nxt, F_EB, ci) = eb + c1E; TB(nxt, F_EE, ci) = ee; }
          if (EMIT && full) {
            Node nd;
            nd.dBase = base; nd.nD = nD; nd.nE = nE; nd.last = -1; nd.sTop = 1; nd.nBlk = 0;
            nd.stkOff = 2 * dpre + 4 * gid; nd.blkOff = blkPair + 2 * base + 8 * gid; nd.stkCap = 2 * nD + 4; nd.blkCap = 2 * (nD + nE) + 8;
            nd.eLast = 0;                                      // (written in F below, by the element that is the head of Ei[nE - 1])
            nodesR[gid] = nd;
            stkR[nd.stkOff] = make_int2(-1, (int)nE + 1);     // dummy pair (DivideSubByRow1.h:470)
          }
        }
        nNodesTot += totF; nEntries += totEnt; sumD += totD; nNext += totC;
      }
      if (outgrown) break;
      SYNC();
      BTICK(4);
      // F: node index of every element for the next level; emit Di / Ei and the visit records
      {
        // (the pass reads ln[P + .], the tables, ph, lpn and the points; it writes ln[.] below P, the entries and the level's visit plane: nothing it reads)
        constexpr int UF = 2;
        for (int j0 = 0; j0 < Pf; j0 += UF * NT) {
          uint32_t k2v[UF], le[UF], ls[UF], ch[UF], gidv[UF], bg[UF], c1[UF], nNE[UF], nND[UF], bs[UF], p0v[UF], p1v[UF], pbg[UF], posv[UF], tq[UF], tt[UF];
#pragma unroll
          for (int u = 0; u < UF; u++) {
            const int j = j0 + u * NT + tid;
            k2v[u] = NONE; p0v[u] = 0; p1v[u] = 0; posv[u] = 0;
            if (j < Pf) { k2v[u] = LN(P + j); if (EMIT) { p0v[u] = (uint32_t)ph[j]; p1v[u] = (uint32_t)ph[j + 1]; posv[u] = lpn[j]; } }
          }
#pragma unroll
          for (int u = 0; u < UF; u++) {
            const int j = j0 + u * NT + tid;
            const bool isS = j < nS;
            le[u] = 0; ls[u] = 0; ch[u] = 0; gidv[u] = NONE; bg[u] = 0; c1[u] = 0; nNE[u] = 0; nND[u] = 0; bs[u] = 0; tq[u] = 0; tt[u] = 0;
            if (k2v[u] != NONE) {
              const uint32_t k = k2v[u] >> 1, side = k2v[u] & 1;
              le[u] = TB(cur, F_LE, k); ls[u] = TB(cur, F_LS, k); ch[u] = side == 0 ? TM(T_CH0, k) : TM(T_CH1, k); gidv[u] = TM(T_GID, k);
              if (EMIT) {
                bg[u] = isS ? TB(cur, F_SB, k) : TB(cur, F_EB, k); c1[u] = isS ? TM(T_C1S, k) : TM(T_C1E, k);
                nNE[u] = TM(T_NE, k); nND[u] = TM(T_ND, k); bs[u] = TM(T_BASE, k);
                tq[u] = hq[posv[u]]; tt[u] = ht[posv[u]];
              }
            }
          }
#pragma unroll
          for (int u = 0; u < UF; u++) {
            pbg[u] = 0;
            if (EMIT && k2v[u] != NONE) {
              const uint32_t side = k2v[u] & 1;
              const bool leaf = le[u] - ls[u] == 1;
              uint32_t beg = bg[u];
              if (!leaf && side == 1) beg += c1[u];
              bg[u] = beg;
              pbg[u] = (uint32_t)ph[beg];
            }
          }
#pragma unroll
          for (int u = 0; u < UF; u++) {
            const int j = j0 + u * NT + tid;
            if (j >= Pf) continue;
            if (k2v[u] == NONE) { ln[j] = INONE; continue; }
            const uint32_t side = k2v[u] & 1;
            const bool leaf = le[u] - ls[u] == 1;
            ln[j] = (IT)(leaf ? NONE : ch[u]);
            const uint32_t gid = gidv[u];
            const bool isS = j < nS;
            const bool in = leaf || (int)side == (isS ? eSide : dSide);
            if (in && gid != NONE) {
              if (!EMIT) nVisits++;
              else {
                const uint32_t head = p1v[u] - p0v[u];
                const uint32_t grp = p0v[u] - pbg[u] + head - 1;
                const uint32_t n = isS ? nNE[u] : nND[u];
                const uint32_t idx = desc ? n - 1 - grp : grp;
                const uint32_t ent = bs[u] + (isS ? nND[u] + idx : idx);
                const uint32_t pos = posv[u];
                if (head) {
                  const long long dgv = back ? (long long)tt[u] + tq[u] : (long long)tt[u] - tq[u];   // (the element's diagonal, from its point: ldn may hold 32 bits of it)
                  entR[ent].val = dgv;
                  if (isS && idx == n - 1) nodesR[gid].eLast = dgv;
                }
                visL[pos] = make_uint2(gid, idx);
              }
            }
          }
        }
      }
      SYNC();
      BTICK(5);
      // G: Db / Eb in closed form (Decide_Eb_Db_*), values and back pointers zeroed
      if (EMIT) {
        // (reads: ln[P + .], the tables, ph, the .val fields of the level's entries (written by F, above the barrier); writes: the .b / .v fields, Ei[Db], the back
        // pointers -- so the binary searches of UG chunks run side by side, a probe of each per round)
        constexpr int UG = 2;
        for (int j0 = 0; j0 < Pf; j0 += UG * NT) {
          uint32_t k2v[UG], gidv[UG], le[UG], ls[UG], bg[UG], c1[UG], nDv[UG], nEv[UG], bs[UG], p0v[UG], p1v[UG], pbg[UG];
          bool on[UG];
#pragma unroll
          for (int u = 0; u < UG; u++) {
            const int j = j0 + u * NT + tid;
            k2v[u] = NONE; p0v[u] = 0; p1v[u] = 0;
            if (j < Pf) { k2v[u] = LN(P + j); p0v[u] = (uint32_t)ph[j]; p1v[u] = (uint32_t)ph[j + 1]; }
          }
#pragma unroll
          for (int u = 0; u < UG; u++) {
            const int j = j0 + u * NT + tid;
            const bool isS = j < nS;
            gidv[u] = NONE; le[u] = 0; ls[u] = 0; bg[u] = 0; c1[u] = 0; nDv[u] = 0; nEv[u] = 0; bs[u] = 0;
            if (k2v[u] != NONE && p1v[u] != p0v[u]) {
              const uint32_t k = k2v[u] >> 1;
              gidv[u] = TM(T_GID, k); le[u] = TB(cur, F_LE, k); ls[u] = TB(cur, F_LS, k);
              bg[u] = isS ? TB(cur, F_SB, k) : TB(cur, F_EB, k); c1[u] = isS ? TM(T_C1S, k) : TM(T_C1E, k);
              nDv[u] = TM(T_ND, k); nEv[u] = TM(T_NE, k); bs[u] = TM(T_BASE, k);
            }
          }
#pragma unroll
          for (int u = 0; u < UG; u++) {
            const int j = j0 + u * NT + tid;
            const bool isS = j < nS;
            const uint32_t side = k2v[u] & 1;
            const bool leaf = le[u] - ls[u] == 1;
            on[u] = k2v[u] != NONE && p1v[u] != p0v[u] && gidv[u] != NONE && (leaf || (int)side == (isS ? eSide : dSide));
            pbg[u] = 0;
            if (on[u]) { uint32_t beg = bg[u]; if (!leaf && side == 1) beg += c1[u]; pbg[u] = (uint32_t)ph[beg]; }
          }
          uint32_t entv[UG], mv[UG], lo[UG], cnt[UG]; long long xv[UG]; const Ent* opp[UG];
#pragma unroll
          for (int u = 0; u < UG; u++) {
            const int j = j0 + u * NT + tid;
            const bool isS = j < nS;
            const uint32_t grp = p0v[u] - pbg[u];
            const uint32_t n = isS ? nEv[u] : nDv[u];
            const uint32_t idx = desc ? n - 1 - grp : grp;
            entv[u] = bs[u] + (isS ? nDv[u] + idx : idx);
            opp[u] = entR + bs[u] + (isS ? 0 : nDv[u]);
            mv[u] = isS ? nDv[u] : nEv[u];
            xv[u] = on[u] ? entR[entv[u]].val : 0;
            lo[u] = 0; cnt[u] = on[u] ? mv[u] : 0;
          }
          // D entry: asc  #{Ei < x}   desc #{Ei >= x};   E entry: asc #{Di <= x}   desc #{Di > x}
          // (the lists are sorted and the predicate holds on a prefix: two steps of the bisection per round -- the probe in the middle and the two probes its outcome can lead
          // to are asked for together; a round is a trip to L2 and a level of the decomposition has a dozen of these searches per element group)
          while (true) {
            bool any = false;
#pragma unroll
            for (int u = 0; u < UG; u++) any |= cnt[u] > 0;
            if (!any) break;
            long long vM[UG], vL[UG], vR[UG];
#pragma unroll
            for (int u = 0; u < UG; u++) {
              const uint32_t step = cnt[u] >> 1, it = lo[u] + step, cntT = cnt[u] > 0 ? cnt[u] - step - 1 : 0;
              vM[u] = cnt[u] > 0 ? opp[u][it].val : 0;
              vL[u] = step > 0 ? opp[u][lo[u] + (step >> 1)].val : 0;
              vR[u] = cntT > 0 ? opp[u][it + 1 + (cntT >> 1)].val : 0;
            }
#pragma unroll
            for (int u = 0; u < UG; u++) {
              if (cnt[u] == 0) continue;
              const bool isS = j0 + u * NT + tid < nS;
              auto go = [&](long long v) { return isS ? (desc ? v > xv[u] : v <= xv[u]) : (desc ? v >= xv[u] : v < xv[u]); };
              const uint32_t step = cnt[u] >> 1, it = lo[u] + step;
              if (go(vM[u])) {
                lo[u] = it + 1; cnt[u] -= step + 1;
                if (cnt[u] > 0) { const uint32_t s2 = cnt[u] >> 1; if (go(vR[u])) { lo[u] += s2 + 1; cnt[u] -= s2 + 1; } else cnt[u] = s2; }
              } else {
                cnt[u] = step;
                if (cnt[u] > 0) { const uint32_t s2 = cnt[u] >> 1; if (go(vL[u])) { lo[u] += s2 + 1; cnt[u] -= s2 + 1; } else cnt[u] = s2; }
              }
            }
          }
#pragma unroll
          for (int u = 0; u < UG; u++) {
            if (!on[u]) continue;
            const bool isS = j0 + u * NT + tid < nS;
            const uint32_t ent = entv[u], m = mv[u];
            entR[ent].b = isS ? (int32_t)lo[u] - 1 : (lo[u] == m ? -1 : (int32_t)lo[u]);
            if (!isS) edR[ent] = lo[u] == m ? 0 : opp[u][lo[u]].val;        // Ei[Db[d]]
            // (Ev[] is written but never read by the reference, and Db[Eb + 1] -- which the flush at the end of Maximization tests against the top pair's boundary,
            // :450 -- is never needed: that boundary is n or n + 1, see sdp_process_wg)
            entR[ent].v = 0.f; apR[ent] = 0;
          }
        }
      }
      nNodes = nNext; cur = nxt;
      SYNC();
      BTICK(6);
    }
  }
  if (bstat && tid == 0) { for (int k = 0; k < 8; k++) atomicAdd(a.stat + k, s_bt[k]); atomicAdd(a.stat + 8, (unsigned long long)P); }
  for (int o = 32; o > 0; o >>= 1) nVisits += __shfl_xor(nVisits, o);
  if (NW > 1) {
    if (lane == 0) s_w[0][wave] = (int)nVisits;
    __syncthreads();
    nVisits = 0;
    for (int w = 0; w < NW; w++) nVisits += (uint32_t)s_w[0][w];
  }
  if (tid == 0) {
    if (!EMIT) { a.cntEntries[rr] = nEntries; a.cntNodes[rr] = nNodesTot; a.cntD[rr] = sumD; a.cntV[rr] = nVisits; a.cntRC[rr] = (uint32_t)max(R, C); a.lines[2 * rr] = (uint32_t)R; a.lines[2 * rr + 1] = (uint32_t)C; }
    else { a.cntV[rr] = nEntries; a.cntRC[rr] = (uint32_t)max(R, C); }      // (what the read really has; its rows / columns for the choice of the ProcessPoint kernel)
    if (overflow) atomicOr(&a.status[r], (uint32_t)LRA_ST_RANGE);             // more than 2^(LV-1) distinct rows / columns (or a level beyond the read's visit planes)
    if (outgrown) atomicOr(&a.status[r], (uint32_t)LRA_ST_CAPACITY);
  }
#undef TB
#undef TM
#undef BTICK
}

// The one-wave-per-read builds of a launch: reads [from, to) of `order` (largest first).  Those of at most 512 points keep their element arrays in LDS
// (three sizes of LDS request, so that small reads do not pay for large ones' occupancy); the rest work from the scratch arena.
template <bool EMIT>
void small_builds(lra_ctx* ctx, const BuildArgs& ba, const uint32_t* d_order, const std::vector<uint32_t>& h_order, const uint64_t* h_pt, int from, int to) {
  hipStream_t st = ctx->stream;
  auto pts = [&](int i) { return (long)(h_pt[h_order[i] + 1] - h_pt[h_order[i]]); };
  int at = from;
  // (measured: at 28 KB -- up to 1024 points -- five waves per CU are slower from LDS than 32 from the arena; up to 768 points is a wash)
  const long caps[3] = {512, 256, 128};
  int cut[4];                                                            // [from, cut0): arena;  [cut0, cut1): <= 512;  [cut1, cut2): <= 256;  [cut2, to): <= 128
  for (int c = 0; c < 3; c++) { while (at < to && pts(at) > caps[c]) at++; cut[c] = at; }
  cut[3] = to;
  if (cut[0] > from) {                                                   // arena: 16-bit indices below 16384 points (2 x node index + side must fit)
    int mid = from;
    while (mid < cut[0] && pts(mid) >= 16384) mid++;
    if (mid > from) { BuildArgs bb = ba; bb.order = d_order + from; hipLaunchKernelGGL((sdp_build<EMIT, 1, 0>), dim3(mid - from), dim3(64), 0, st, bb); }
    if (cut[0] > mid) {
      BuildArgs bb = ba; bb.order = d_order + mid;
      // waves per SIMD the register budget is set for: 8; beside another batch's half (two-stage batches) 6 -- fewer, fatter waves leave the other half's launches room
      // (two-stage step 952 -> 937 ms; in the one call 8 is the faster one)
      const bool occ6 = ctx->pipelined;
      if (bb.stat) { if (occ6) hipLaunchKernelGGL((sdp_build<EMIT, 1, 2, 6, true>), dim3(cut[0] - mid), dim3(64), 0, st, bb); else hipLaunchKernelGGL((sdp_build<EMIT, 1, 2, 8, true>), dim3(cut[0] - mid), dim3(64), 0, st, bb); }
      else if (occ6) hipLaunchKernelGGL((sdp_build<EMIT, 1, 2, 6>), dim3(cut[0] - mid), dim3(64), 0, st, bb);
      else hipLaunchKernelGGL((sdp_build<EMIT, 1, 2>), dim3(cut[0] - mid), dim3(64), 0, st, bb);
    }
  }
  for (int c = 0; c < 3; c++) {
    const int n = cut[c + 1] - cut[c];
    if (n <= 0) continue;
    BuildArgs bb = ba; bb.order = d_order + cut[c];
    hipLaunchKernelGGL((sdp_build<EMIT, 1, 1>), dim3(n), dim3(64), (size_t)(28 * caps[c] + 32), st, bb);
  }
}

}  // namespace

namespace lra_sdp {

void launch_wg_builds(bool emit, hipStream_t st, const BuildArgs& ba, int n) {
  if (emit) hipLaunchKernelGGL((sdp_build<true, 16>), dim3(n), dim3(1024), 0, st, ba);
  else hipLaunchKernelGGL((sdp_build<false, 16>), dim3(n), dim3(1024), 0, st, ba);
}
void launch_small_builds(bool emit, lra_ctx* ctx, const BuildArgs& ba, const uint32_t* d_order, const std::vector<uint32_t>& h_order, const uint64_t* h_pt, int from, int to) {
  if (emit) small_builds<true>(ctx, ba, d_order, h_order, h_pt, from, to);
  else small_builds<false>(ctx, ba, d_order, h_order, h_pt, from, to);
}

}  // namespace lra_sdp

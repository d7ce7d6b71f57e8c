// lra_amd/csrc/sdp_trace.hip -- the sparse DP's back end (sdp.h lists the files): the value order's keys, TraceBack's predecessor per fragment, and sdp_trace
// (TraceBack + DecidePrimaryChains, one lane per read).  gfx950 only.
#include "sdp.h"

using namespace lra_sdp;

namespace {

// ---- value order, TraceBack, DecidePrimaryChains ------------------------------------------------------------------------
__global__ void k_valkeys(uint64_t f0, uint64_t n, const float* __restrict__ fval, const uint32_t* __restrict__ fragRead,
                          const uint64_t* __restrict__ fragOff, uint64_t* okey, uint32_t* opay) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t g = f0 + i;
  okey[g] = (uint64_t)(0xFFFFFFFFu - __float_as_uint(fval[g]));         // Fragment_valueOrder: value descending (values are >= 0)
  opay[g] = (uint32_t)(g - fragOff[fragRead[g]]);
}

// TraceBack's step Dp[Ep[prev_ind]] of sub-problem prev_sub, resolved for every fragment at once (the chain walk then chases one pointer
// per anchor instead of four dependent loads); taken after ProcessPoint has finished, as the reference's trace back reads it
__global__ void k_pred(uint64_t f0, uint64_t n, int r0, const uint32_t* __restrict__ fragRead, const uint32_t* __restrict__ fprevNode,
                       const uint32_t* __restrict__ fprevInd, const uint32_t* __restrict__ status, const ReadArena* __restrict__ ra, uint32_t* fpred) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t g = f0 + i;
  const uint32_t r = fragRead[g];
  uint32_t pred = NONE;
  const uint32_t pn = fprevNode[g], pi = fprevInd[g];
  if (!status[r] && pn != NONE && pi != NONE) {
    const ReadArena A = ra[(int)r - r0];
    const Node* nodesR = (const Node*)arena_ptr(A.base);
    const uint32_t* apR = (const uint32_t*)(arena_ptr(A.base) + A.apOff);
    const Node nd = nodesR[pn];
    pred = apR[nd.dBase + apR[nd.dBase + nd.nD + pi]];
  }
  fpred[g] = pred;
}

constexpr int TRACE_LANES = 16;           // a serial walk with dependent loads per read: fewer lanes per wave, more waves
__global__ void __launch_bounds__(64) sdp_trace(TraceArgs a) {
  if (threadIdx.x >= TRACE_LANES) return;
  const int rr = blockIdx.x * TRACE_LANES + threadIdx.x;
  if (rr >= a.n) return;
  const int r = a.r0 + rr;
  const uint64_t f0 = a.fragOff[r];
  const int total = (int)(a.fragOff[r + 1] - f0);
  a.nChains[r] = 0;
  if (total == 0 || a.status[r]) return;
  if (a.single) {                                                        // SparseDP.h:2417-2434: first anchor of maximal value, plain TraceBack :1521
    float maxv = 0; uint32_t i = 0;
    for (int l = 0; l < total; l++) if (a.fval[f0 + l] > maxv) { maxv = a.fval[f0 + l]; i = l; }
    uint32_t len = 0;
    a.ccl[f0] = i; len = 1;
    uint32_t nx;
    while ((nx = a.fpred[f0 + i]) != NONE && len < (uint32_t)total) {
      a.clink[f0 + len - 1] = (a.fflags[f0 + i] & 2) ? 0 : 1;
      i = nx;
      a.ccl[f0 + len] = i; len++;
    }
    a.clink[f0 + len - 1] = 0;
    const int slot = r * a.numAln;
    a.chainStart[slot] = f0; a.chainLen[slot] = len; a.chainValue[slot] = maxv;
    a.chainBox[4 * slot] = 0; a.chainBox[4 * slot + 1] = 0; a.chainBox[4 * slot + 2] = 0; a.chainBox[4 * slot + 3] = 0;
    for (uint64_t k = f0; k < f0 + len; k++) {
      const uint32_t lf = a.ccl[k];
      a.cq[k] = a.fq[f0 + lf]; a.ct[k] = a.ft[f0 + lf]; a.clen[k] = a.flen[f0 + lf]; a.cstrand[k] = a.fstrand[f0 + lf];
      a.can[k] = a.fai[f0 + lf]; a.ccl[k] = a.fcl[f0 + lf];
    }
    a.nChains[r] = 1;
    return;
  }
  const int readLen = (int)(a.read_off[r + 1] - a.read_off[r]);
  const float best = a.fval[f0 + a.opay[f0]];
  const float thres = a.boxes ? fmaxf(a.alnthres * best, best - (float)(130 * a.globalK)) : a.alnthres * best;   // :1592 / :1663
  int nCh = 0, fv = 0;
  uint64_t out = f0;                                                     // chains are written back to back into the read's fragment range
  uint32_t c0TS = 0, c0TE = 0;
  while ((a.boxes || nCh < a.numAln) && fv < total && a.fval[f0 + a.opay[f0 + fv]] >= thres) {
    uint32_t i = a.opay[f0 + fv];
    const float firstVal = a.fval[f0 + i];
    // TraceBack with `used` (:1351-1438); the chain is written at out.. and rolled back if it runs into a used anchor
    uint32_t len = 0;
    bool abandoned = false;
    if (a.used[f0 + i] == 0) {
      a.ccl[out] = i; len = 1; a.used[f0 + i] = 1;
      uint32_t nx;
      while ((nx = a.fpred[f0 + i]) != NONE) {                          // Dp[Ep[prev_ind]] of sub-problem prev_sub (k_pred)
        if (a.used[f0 + nx] == 0) { a.clink[out + len - 1] = (a.fflags[f0 + i] & 2) ? 0 : 1; i = nx; }
        else { abandoned = true; break; }
        a.ccl[out + len] = i; len++; a.used[f0 + i] = 1;                 // (the reference tests used[i] again here: it has just seen it clear)
      }
      if (abandoned) { for (uint32_t k = 0; k < len; k++) a.used[f0 + a.ccl[out + k]] = 0; len = 0; }
    }
    if (len != 0 && a.boxes) {                                           // :1607-1650
      uint32_t f = a.ccl[out], l = a.ccl[out + len - 1];
      uint32_t QEnd = a.fqe[f0 + f], TEnd = a.fte[f0 + f], QStart = a.fq[f0 + l], TStart = a.ft[f0 + l];
      int na = 0;
      for (uint32_t k = 0; k < len; k++) {
        f = a.ccl[out + k];
        QEnd = max(QEnd, a.fqe[f0 + f]); TEnd = max(TEnd, a.fte[f0 + f]);
        QStart = min(QStart, a.fq[f0 + f]); TStart = min(TStart, a.ft[f0 + f]);
        if (a.numAnchors) na += a.numAnchors[f0 + f];                    // ComputeNumOfAnchors :1577
      }
      if ((double)((float)(QEnd - QStart) / readLen) > 0.005) {
        if (nCh >= a.numAln) break;
        const int slot = r * a.numAln + nCh;
        a.chainStart[slot] = out; a.chainLen[slot] = len; a.chainValue[slot] = firstVal; a.chainNum[slot] = na;
        a.chainBox[4 * slot] = QStart; a.chainBox[4 * slot + 1] = QEnd; a.chainBox[4 * slot + 2] = TStart; a.chainBox[4 * slot + 3] = TEnd;
        a.clink[out + len - 1] = 0;
        nCh++;
        out += len;
      } else break;
    } else if (len != 0) {
      uint32_t f = a.ccl[out], l = a.ccl[out + len - 1];
      uint32_t QEnd = a.fq[f0 + f] + a.flen[f0 + f], QStart = a.fq[f0 + l], TEnd = a.ft[f0 + f] + a.flen[f0 + f], TStart = a.ft[f0 + l];
      for (uint32_t k = 0; k < len; k++) {
        f = a.ccl[out + k];
        QEnd = max(QEnd, a.fq[f0 + f] + (uint32_t)a.flen[f0 + f]);
        QStart = min(QStart, a.fq[f0 + f]);
        TStart = min(TStart, a.ft[f0 + f]);
        TEnd = min(TEnd, a.ft[f0 + f] + (uint32_t)a.flen[f0 + f]);       // min, as the reference has it (:1694)
      }
      if (len >= 3 && QEnd > QStart && (double)((float)(QEnd - QStart) / readLen) > 0.005 && QEnd - QStart >= 200) {
        bool push = false;
        if (nCh == 0) push = true;
        else {                                                           // chains[0].OverlapsOnT(TStart, TEnd, 0.05f)  Chain.h:261
          int ovp = 0;
          if (TStart >= c0TS && TStart < c0TE) ovp = (int)(min(TEnd, c0TE) - TStart);
          else if (TEnd > c0TS && TEnd <= c0TE) ovp = (int)(TEnd - max(TStart, c0TS));
          else if (TStart < c0TS && TEnd > c0TE) ovp = (int)(c0TE - c0TS);
          const float denomA = (float)(c0TE - c0TS);
          push = (ovp / denomA <= 0.05f);
        }
        if (push) {
          const int slot = r * a.numAln + nCh;
          a.chainStart[slot] = out; a.chainLen[slot] = len; a.chainValue[slot] = firstVal;
          a.chainBox[4 * slot] = QStart; a.chainBox[4 * slot + 1] = QEnd; a.chainBox[4 * slot + 2] = TStart; a.chainBox[4 * slot + 3] = TEnd;
          a.clink[out + len - 1] = 0;
          if (nCh == 0) { c0TS = TStart; c0TE = TEnd; }
          nCh++;
          out += len;
        }
      } else break;
    }
    fv++;
  }
  // local fragment index -> (cluster, anchor)
  for (uint64_t k = f0; k < out; k++) {
    const uint32_t lf = a.ccl[k];
    a.cq[k] = a.fq[f0 + lf]; a.ct[k] = a.ft[f0 + lf]; a.clen[k] = a.flen[f0 + lf]; a.cstrand[k] = a.fstrand[f0 + lf];
    a.can[k] = a.fai[f0 + lf]; a.ccl[k] = a.fcl[f0 + lf];
  }
  a.nChains[r] = (uint32_t)nCh;
}

}  // namespace

namespace lra_sdp {

void launch_valkeys(hipStream_t st, uint64_t f0, uint64_t n, const float* fval, const uint32_t* fragRead, const uint64_t* fragOff, uint64_t* okey, uint32_t* opay) {
  hipLaunchKernelGGL(k_valkeys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, f0, n, fval, fragRead, fragOff, okey, opay);
}
void launch_pred(hipStream_t st, uint64_t f0, uint64_t n, int r0, const uint32_t* fragRead, const uint32_t* fprevNode, const uint32_t* fprevInd, const uint32_t* status,
                 const ReadArena* ra, uint32_t* fpred) {
  hipLaunchKernelGGL(k_pred, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, f0, n, r0, fragRead, fprevNode, fprevInd, status, ra, fpred);
}
void launch_trace(hipStream_t st, const TraceArgs& ta) {
  hipLaunchKernelGGL(sdp_trace, dim3((ta.n + TRACE_LANES - 1) / TRACE_LANES), dim3(64), 0, st, ta);
}

}  // namespace lra_sdp

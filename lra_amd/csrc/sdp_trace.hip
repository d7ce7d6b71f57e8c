// lra_amd/csrc/sdp_trace.hip -- the sparse DP's back end (sdp.h lists the files): the value order's keys, TraceBack's predecessor per fragment, and sdp_trace
// (TraceBack + DecidePrimaryChains, one wave per read).  gfx950 only.
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

// ---- sdp_trace: a wave per read.  What the chain walk reads (fpred, and in general mode the value order and `used`) is staged in LDS with wave-wide loads for reads of
// up to TRACE_CAP anchors; lane 0 chases there, at LDS latency instead of a memory round trip per anchor, and writes the chain's local indices to LDS; the maximum,
// the per-chain boxes, the links and the closing gather are wave-wide passes.  The decisions are the sequential ones of the reference, taken wave-uniformly.  A read
// beyond TRACE_CAP (or one whose fpred / opay do not fit the 16-bit copies) keeps the walk on lane 0 from memory; its gather is wave-wide all the same.
constexpr uint16_t PRED_NONE = 0xFFFFu, CHAIN_END = 0x8000u;   // (local indices are < TRACE_CAP < CHAIN_END)
template <bool SINGLE> struct TraceLds {
  uint16_t pred[TRACE_CAP];                // fpred
  uint16_t chain[TRACE_CAP];               // the chains' local fragment indices, back to back as ccl holds them; general mode: CHAIN_END marks a kept chain's last anchor
  uint16_t ord[SINGLE ? 1 : TRACE_CAP];    // opay (general mode)
  uint32_t used[SINGLE ? 1 : TRACE_CAP / 32];   // general mode, a bit per anchor
};
static_assert(TRACE_CAP % 64 == 0 && TRACE_CAP < CHAIN_END && sizeof(TraceLds<false>) <= 16384, "a wave's LDS stays within 16 KB");

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) { for (int o = 32; o; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o)); return v; }
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) { for (int o = 32; o; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o)); return v; }
__device__ __forceinline__ int wave_sum_i32(int v) { for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o); return v; }
__device__ __forceinline__ uint32_t first_lane(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// local fragment index -> (cluster, anchor), and the anchor itself for the split-chain stage
__device__ __forceinline__ void gather_anchor(const TraceArgs& a, uint64_t f0, uint64_t k, uint32_t lf) {
  a.cq[k] = a.fq[f0 + lf]; a.ct[k] = a.ft[f0 + lf]; a.clen[k] = a.flen[f0 + lf]; a.cstrand[k] = a.fstrand[f0 + lf];
  a.can[k] = a.fai[f0 + lf]; a.ccl[k] = a.fcl[f0 + lf];
}

// plain TraceBack (SparseDP.h:1521) from anchor i, one lane from memory -> the chain's length; ccl holds local indices
__device__ uint32_t single_walk_lane(const TraceArgs& a, uint64_t f0, int total, uint32_t i) {
  uint32_t len = 0;
  a.ccl[f0] = i; len = 1;
  uint32_t nx;
  while ((nx = a.fpred[f0 + i]) != NONE && len < (uint32_t)total) {
    a.clink[f0 + len - 1] = (a.fflags[f0 + i] & 2) ? 0 : 1;
    i = nx;
    a.ccl[f0 + len] = i; len++;
  }
  a.clink[f0 + len - 1] = 0;
  return len;
}

// DecidePrimaryChains, one lane from memory -> the number of chains; out: the end of the chains written back to back from f0 (ccl holds local indices)
template <bool BOXES> __device__ int general_walk_lane(const TraceArgs& a, int r, uint64_t f0, int total, int readLen, float thres, uint64_t& out) {
  int nCh = 0, fv = 0;
  out = f0;                                                              // chains are written back to back into the read's fragment range
  uint32_t c0TS = 0, c0TE = 0;
  while ((BOXES || nCh < a.numAln) && fv < total && a.fval[f0 + a.opay[f0 + fv]] >= thres) {
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
    if (len != 0 && BOXES) {                                           // :1607-1650
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
  return nCh;
}

template <bool SINGLE, bool BOXES>        // the single-cluster drivers' trace, DecidePrimaryChains on clusters and on boxes: a kernel each, so that none carries the others' pointers
__global__ void __launch_bounds__(64) sdp_trace(TraceArgs a) {
  __shared__ TraceLds<SINGLE> s;
  const int lane = threadIdx.x;
  const int r = a.r0 + blockIdx.x;
  const uint64_t f0 = a.fragOff[r];
  const int total = (int)(a.fragOff[r + 1] - f0);
  if (total == 0 || a.status[r]) { if (lane == 0) a.nChains[r] = 0; return; }
  bool staged = total <= TRACE_CAP;
  if (staged) {
    bool bad = false;
    for (int l = lane; l < total; l += 64) {
      const uint32_t p = a.fpred[f0 + l];
      bad |= p != NONE && p >= (uint32_t)total;
      s.pred[l] = p == NONE ? PRED_NONE : (uint16_t)p;
      if (!SINGLE) { const uint32_t o = a.opay[f0 + l]; bad |= o >= (uint32_t)total; s.ord[l] = (uint16_t)o; }
    }
    if (!SINGLE)
      for (int b = 0; b < total; b += 64) {
        const uint64_t m = __ballot(b + lane < total && a.used[f0 + b + lane] != 0);
        if (lane == 0) { s.used[b >> 5] = (uint32_t)m; s.used[(b >> 5) + 1] = (uint32_t)(m >> 32); }
      }
    staged = __ballot(bad) == 0;
    wave_sync();
  }
  if (SINGLE) {                                                        // SparseDP.h:2417-2434: first anchor of maximal value, plain TraceBack :1521
    float maxv = 0; uint32_t mi = 0;                                     // per lane over its stride, then across lanes: strict >, the lowest index among equal maxima
    for (int l = lane; l < total; l += 64) { const float v = a.fval[f0 + l]; if (v > maxv) { maxv = v; mi = l; } }
    for (int o = 32; o; o >>= 1) {
      const float ov = __shfl_xor(maxv, o); const uint32_t oi = (uint32_t)__shfl_xor((int)mi, o);
      if (ov > maxv || (ov == maxv && oi < mi)) { maxv = ov; mi = oi; }
    }
    uint32_t len = 0;
    if (staged) {
      if (lane == 0) {
        uint32_t i = mi, nx;
        s.chain[0] = (uint16_t)i; len = 1;
        while ((nx = s.pred[i]) != PRED_NONE && len < (uint32_t)total) { i = nx; s.chain[len] = (uint16_t)i; len++; }
      }
      len = first_lane(len);
      wave_sync();
      for (uint32_t k = lane; k < len; k += 64) {
        const uint32_t lf = s.chain[k];
        uint8_t lk = 0;
        if (k + 1 < len) lk = (a.fflags[f0 + lf] & 2) ? 0 : 1;
        a.clink[f0 + k] = lk;
        gather_anchor(a, f0, f0 + k, lf);
      }
    } else {
      if (lane == 0) len = single_walk_lane(a, f0, total, mi);
      len = first_lane(len);
      wave_sync();
      for (uint32_t k = lane; k < len; k += 64) gather_anchor(a, f0, f0 + k, a.ccl[f0 + k]);
    }
    if (lane == 0) {
      const int slot = r * a.numAln;
      a.chainStart[slot] = f0; a.chainLen[slot] = len; a.chainValue[slot] = maxv;
      a.chainBox[4 * slot] = 0; a.chainBox[4 * slot + 1] = 0; a.chainBox[4 * slot + 2] = 0; a.chainBox[4 * slot + 3] = 0;
      a.nChains[r] = 1;
    }
    return;
  }
  const int readLen = (int)(a.read_off[r + 1] - a.read_off[r]);
  const float best = a.fval[f0 + a.opay[f0]];
  const float thres = BOXES ? fmaxf(a.alnthres * best, best - (float)(130 * a.globalK)) : a.alnthres * best;   // :1592 / :1663
  if (!staged) {
    uint64_t out = f0; int nCh = 0;
    if (lane == 0) nCh = general_walk_lane<BOXES>(a, r, f0, total, readLen, thres, out);
    const uint32_t outL = first_lane((uint32_t)(out - f0));
    wave_sync();
    for (uint32_t k = lane; k < outL; k += 64) gather_anchor(a, f0, f0 + k, a.ccl[f0 + k]);
    if (lane == 0) a.nChains[r] = (uint32_t)nCh;
    return;
  }
  int nCh = 0, fv = 0;
  uint32_t outL = 0;                                                     // chains are written back to back into the read's fragment range
  uint32_t c0TS = 0, c0TE = 0;
  uint64_t pass = 0;                                                     // value >= thres for the 64 candidates from fv & ~63
  while ((BOXES || nCh < a.numAln) && fv < total) {
    if ((fv & 63) == 0) { const int c = fv + lane; pass = __ballot(c < total && a.fval[f0 + s.ord[c < total ? c : 0]] >= thres); }
    if (!((pass >> (fv & 63)) & 1)) break;
    const uint32_t i0 = s.ord[fv];
    if ((s.used[i0 >> 5] >> (i0 & 31)) & 1) { fv++; continue; }
    // TraceBack with `used` (:1351-1438); the chain is written at outL.. and rolled back if it runs into a used anchor
    uint32_t len = 0;
    if (lane == 0) {
      uint32_t i = i0, nx;
      bool abandoned = false;
      s.chain[outL] = (uint16_t)i; len = 1; s.used[i >> 5] |= 1u << (i & 31);
      while ((nx = s.pred[i]) != PRED_NONE) {                            // Dp[Ep[prev_ind]] of sub-problem prev_sub (k_pred)
        if ((s.used[nx >> 5] >> (nx & 31)) & 1) { abandoned = true; break; }
        i = nx;
        s.chain[outL + len] = (uint16_t)i; len++; s.used[i >> 5] |= 1u << (i & 31);
      }
      if (abandoned) { for (uint32_t k = 0; k < len; k++) { const uint32_t f = s.chain[outL + k]; s.used[f >> 5] &= ~(1u << (f & 31)); } len = 0; }
    }
    len = first_lane(len);
    wave_sync();
    if (len == 0) { fv++; continue; }
    bool push = false;
    uint32_t QEnd = 0, TEnd = BOXES ? 0 : 0xFFFFFFFFu, QStart = 0xFFFFFFFFu, TStart = 0xFFFFFFFFu;
    int na = 0;
    if (BOXES) {                                                       // :1607-1650
      for (uint32_t k = lane; k < len; k += 64) {
        const uint32_t f = s.chain[outL + k];
        QEnd = max(QEnd, a.fqe[f0 + f]); TEnd = max(TEnd, a.fte[f0 + f]);
        QStart = min(QStart, a.fq[f0 + f]); TStart = min(TStart, a.ft[f0 + f]);
        if (a.numAnchors) na += a.numAnchors[f0 + f];                    // ComputeNumOfAnchors :1577
      }
      QEnd = wave_max_u32(QEnd); TEnd = wave_max_u32(TEnd); QStart = wave_min_u32(QStart); TStart = wave_min_u32(TStart); na = wave_sum_i32(na);
      if (!((double)((float)(QEnd - QStart) / readLen) > 0.005)) break;
      if (nCh >= a.numAln) break;
      push = true;
    } else {
      for (uint32_t k = lane; k < len; k += 64) {
        const uint32_t f = s.chain[outL + k];
        const uint32_t q = a.fq[f0 + f], t = a.ft[f0 + f], ln = (uint32_t)a.flen[f0 + f];
        QEnd = max(QEnd, q + ln);
        QStart = min(QStart, q);
        TStart = min(TStart, t);
        TEnd = min(TEnd, t + ln);                                        // min, as the reference has it (:1694)
      }
      QEnd = wave_max_u32(QEnd); TEnd = wave_min_u32(TEnd); QStart = wave_min_u32(QStart); TStart = wave_min_u32(TStart);
      if (!(len >= 3 && QEnd > QStart && (double)((float)(QEnd - QStart) / readLen) > 0.005 && QEnd - QStart >= 200)) break;
      if (nCh == 0) push = true;
      else {                                                             // chains[0].OverlapsOnT(TStart, TEnd, 0.05f)  Chain.h:261
        int ovp = 0;
        if (TStart >= c0TS && TStart < c0TE) ovp = (int)(min(TEnd, c0TE) - TStart);
        else if (TEnd > c0TS && TEnd <= c0TE) ovp = (int)(TEnd - max(TStart, c0TS));
        else if (TStart < c0TS && TEnd > c0TE) ovp = (int)(c0TE - c0TS);
        const float denomA = (float)(c0TE - c0TS);
        push = (ovp / denomA <= 0.05f);
      }
    }
    if (push) {
      if (lane == 0) {
        const int slot = r * a.numAln + nCh;
        a.chainStart[slot] = f0 + outL; a.chainLen[slot] = len; a.chainValue[slot] = a.fval[f0 + i0];
        if (BOXES) a.chainNum[slot] = na;
        a.chainBox[4 * slot] = QStart; a.chainBox[4 * slot + 1] = QEnd; a.chainBox[4 * slot + 2] = TStart; a.chainBox[4 * slot + 3] = TEnd;
        s.chain[outL + len - 1] |= CHAIN_END;
      }
      if (!BOXES && nCh == 0) { c0TS = TStart; c0TE = TEnd; }
      nCh++;
      outL += len;
    }
    fv++;
  }
  wave_sync();
  for (uint32_t k = lane; k < outL; k += 64) {
    const uint32_t e = s.chain[k], lf = e & (CHAIN_END - 1u);
    uint8_t lk = 0;
    if (!(e & CHAIN_END)) lk = (a.fflags[f0 + lf] & 2) ? 0 : 1;
    a.clink[f0 + k] = lk;
    gather_anchor(a, f0, f0 + k, lf);
  }
  if (lane == 0) a.nChains[r] = (uint32_t)nCh;
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
  if (ta.single) hipLaunchKernelGGL((sdp_trace<true, false>), dim3(ta.n), dim3(64), 0, st, ta);
  else if (ta.boxes) hipLaunchKernelGGL((sdp_trace<false, true>), dim3(ta.n), dim3(64), 0, st, ta);
  else hipLaunchKernelGGL((sdp_trace<false, false>), dim3(ta.n), dim3(64), 0, st, ta);
}

}  // namespace lra_sdp

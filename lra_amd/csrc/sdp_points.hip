// lra_amd/csrc/sdp_points.hip -- the sparse DP's small kernels around its three large ones (sdp.h lists the files): counts and offsets per cluster and read, the points
// of every anchor, the gathers behind the sorts, Value[]'s reset for a read that is run again, the gap-cost table, and the layout of the per-read arenas.  gfx950 only.
#include <algorithm>
#include "sdp_process.h"

using namespace lra_sdp;

namespace {

__global__ void k_arena_sizes(int n, int r0, const uint64_t* __restrict__ ptOff, const uint32_t* __restrict__ cntE, const uint32_t* __restrict__ cntN,
                              const uint32_t* __restrict__ cntD, const uint32_t* __restrict__ lines, ReadArena* ra, uint64_t* bytes,
                              const uint32_t* __restrict__ order, int shift) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  const int rr = (int)order[b];
  const uint64_t E = cntE[rr], N = cntN[rr], D = cntD[rr], P = ptOff[r0 + rr + 1] - ptOff[r0 + rr];
  ReadArena a;
  a.base = 0;
  uint64_t o = al256(N * sizeof(Node));
  a.entOff = (uint32_t)o; o = al256(o + E * sizeof(Ent));
  a.apOff = (uint32_t)o; o = al256(o + E * 4);
  a.edOff = (uint32_t)o; o = al256(o + E * 8);
  const uint64_t stkPairs = 2 * D + 4 * N + 2, blkPairs = 2 * E + 8 * N + 2, poolPairs = (2 * E + 4096) << shift;
  a.stkOff = (uint32_t)o; a.blkPair = (uint32_t)stkPairs; a.poolPair = (uint32_t)(stkPairs + blkPairs); a.poolPairs = (uint32_t)poolPairs;
  o = al256(o + (stkPairs + blkPairs + poolPairs) * 8);
  // the visit planes: as many as the read's rows / columns give levels -- counted (k_big_lines, the count pass: lines[] != 0), else no more than its points
  const uint32_t nR = lines[2 * rr], nC = lines[2 * rr + 1];
  const uint32_t plR = vis_planes(nR ? nR : P), plC = vis_planes(nC ? nC : P);
  a.visPl = plR | (plC << 8);
  a.visOff = (uint32_t)o; o = al256(o + P * (plR + plC) * sizeof(uint2));
  ra[rr] = a;
  bytes[b] = o;
}
// Sizes WITHOUT the count pass: entries, sub-problems and D entries per point are narrow distributions (measured over the headline batch: 3.2 .. 9.8 entries and 0.3 .. 1.9
// sub-problems per point, D entries 43 .. 56 % of the entries), so a read's blocks are laid out for fE / fN per point and the emit pass checks every level against them; the rare
// read that outgrows its blocks is counted exactly and built again with the reads whose stacks outgrew theirs (attempt 1 of sdp_run).
__global__ void k_arena_estimate(int n, int r0, const uint64_t* __restrict__ ptOff, float fE, float fN, uint32_t* cntE, uint32_t* cntN, uint32_t* cntD) {
  int rr = blockIdx.x * blockDim.x + threadIdx.x;
  if (rr >= n) return;
  const uint64_t P = ptOff[r0 + rr + 1] - ptOff[r0 + rr];
  const uint64_t E = (uint64_t)(fE * (float)P) + 64, N = (uint64_t)(fN * (float)P) + 64;
  cntE[rr] = (uint32_t)std::min<uint64_t>(E, 0xFFFFFFFFull); cntN[rr] = (uint32_t)std::min<uint64_t>(N, 0xFFFFFFFFull); cntD[rr] = (uint32_t)std::min<uint64_t>(E * 6 / 10 + 64, 0xFFFFFFFFull);
}
__global__ void k_arena_bases(int n, const uint64_t* __restrict__ byteOff, ReadArena* ra, const uint32_t* __restrict__ order, char* arena) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < n) ra[order[b]].base = (uint64_t)(uintptr_t)(arena + byteOff[b]);
}
__global__ void k_visit_clear(const ReadArena* __restrict__ ra, const uint64_t* __restrict__ byteOff, const uint32_t* __restrict__ order) {
  const int b = blockIdx.x;
  const ReadArena A = ra[order[b]];
  uint4* p = (uint4*)(arena_ptr(A.base) + A.visOff);
  const uint64_t n = (byteOff[b + 1] - byteOff[b] - A.visOff) / 16;
  for (uint64_t i = threadIdx.x; i < n; i += blockDim.x) p[i] = make_uint4(NONE, NONE, NONE, NONE);
}

// The distinct rows and columns (GetRowInfo / GetColInfo) of the reads a launch gives a workgroup each, ahead of their build: the maximum picks the sdp_process_wg
// variant, so that the workgroup ProcessPoint launch can follow the large reads' build on its side stream without a word from the host in between.
__global__ void k_big_lines(int r0, const uint32_t* __restrict__ order, const uint64_t* __restrict__ ptOff, const uint32_t* __restrict__ hq, const uint32_t* __restrict__ ht,
                            const uint32_t* __restrict__ h2, uint32_t* maxLines, uint32_t* lines) {
  const int rr = (int)order[blockIdx.x], r = r0 + rr;
  const uint64_t p0 = ptOff[r];
  const int P = (int)(ptOff[r + 1] - p0);
  const uint32_t* q = hq + p0; const uint32_t* t = ht + p0; const uint32_t* c = h2 + p0;
  uint32_t R = 0, C = 0;
  for (int i = threadIdx.x; i < P; i += blockDim.x) { R += (i == 0 || q[i] != q[i - 1]); C += (i == 0 || t[c[i]] != t[c[i - 1]]); }
  for (int o = 32; o > 0; o >>= 1) { R += __shfl_xor(R, o); C += __shfl_xor(C, o); }
  __shared__ uint32_t sR, sC;
  if (threadIdx.x == 0) { sR = 0; sC = 0; }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { atomicAdd(&sR, R); atomicAdd(&sC, C); }
  __syncthreads();
  if (threadIdx.x == 0) { atomicMax(maxLines, max(sR, sC)); lines[2 * rr] = sR; lines[2 * rr + 1] = sC; }   // (lines[]: k_arena_sizes lays out the read's visit planes from them)
}

// ---- counting / point generation ------------------------------------------------------------------------------------
__global__ void k_cluster_counts(uint64_t nc, const uint32_t* __restrict__ c_count, uint32_t* fragCnt, uint32_t* ptCnt, int single) {
  uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  if (!c_count) { fragCnt[c] = 1; ptCnt[c] = 4; return; }                  // box mode (SparseDP.h:1959-2018): s1 e1 s2 e2 for every box
  uint32_t n = c_count[c];
  fragCnt[c] = n;
  ptCnt[c] = 2 * n + (single ? 0 : 2 * (n == 0 ? 0 : n == 1 ? 1 : 2));     // SparseDP.h:2159-2166: first and last anchor get the other family's pair too
}

__global__ void k_read_offsets(int n_reads, const uint64_t* __restrict__ cluster_off, const uint64_t* __restrict__ clusFragOff,
                               const uint64_t* __restrict__ clusPtOff, uint64_t* fragOff, uint64_t* ptOff, uint32_t* clusRead,
                               uint32_t* status, uint32_t* nChains) {
  int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r > n_reads) return;
  fragOff[r] = clusFragOff[cluster_off[r]];
  ptOff[r] = clusPtOff[cluster_off[r]];
  if (r < n_reads) {
    for (uint64_t c = cluster_off[r]; c < cluster_off[r + 1]; c++) clusRead[c] = r;
    status[r] = 0; nChains[r] = 0;
  }
}

// anchors -> compact fragment arrays + points in insertion order (SparseDP.h:2152-2169).  Box mode: one thread per cluster (= fragment).  Anchor mode: one WAVE per
// cluster, a lane per anchor -- a merged cluster of a satellite read holds 20 k anchors, and one thread walking them kept the launch at 5-13 ms; an anchor's
// points sit at 2 i (+ 2 behind the first anchor's second pair).
__global__ void k_points(PtArgs a) {
  const bool boxMode = a.qe != nullptr;
  const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t c = boxMode ? gtid : (gtid >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (c >= a.nc) return;
  const uint32_t r = a.clusRead[c];
  const int strand = a.c_strand[c];
  uint64_t g = a.clusFragOff[c], p = a.clusPtOff[c];
  const uint64_t f0 = a.fragOff[r], p0 = a.ptOff[r];
  const uint32_t cl = (uint32_t)(c - a.cluster_off[r]);
  const float rate = a.rate_in ? a.rate_in[r] : a.rate;
  if (a.qe) {                                                          // box mode: the split cluster c is the fragment (SparseDP.h:1959-2018)
    const uint32_t qs = a.q[c], ts = a.t[c], qe = a.qe[c], te = a.te[c];
    const int val = a.len[c];
    a.fq[g] = qs; a.ft[g] = ts; a.fqe[g] = qe; a.fte[g] = te; a.flen[g] = val; a.fcl[g] = cl; a.fai[g] = 0;
    a.fval[g] = val * rate;                                            // Value[ii].val = FragInput[ii].Val*rate (:2084)
    a.fprevNode[g] = NONE; a.fprevInd[g] = NONE; a.fflags[g] = 3; a.used[g] = 0; a.fstrand[g] = (uint8_t)(strand != 0);
    const uint32_t lf = (uint32_t)(g - f0);
    for (int k = 0; k < 4; k++, p++) {                                 // s1 (qs+1,ts+1)  e1 (qe-1,te-1)  s2 (qs+1,te-1)  e2 (qe-1,ts+1)
      const uint8_t ind = (k & 1) ? 0 : 1, inv = k < 2 ? 1 : 0;
      const uint32_t pq = ind ? qs + 1 : qe - 1;
      const uint32_t pt = (k == 0 || k == 3) ? ts + 1 : te - 1;
      a.key1[p] = ((uint64_t)pq << 33) | ((uint64_t)pt << 1) | ind;
      a.pay1[p] = (uint32_t)(p - p0);
      a.iq[p] = pq; a.it[p] = pt; a.ifl[p] = (uint8_t)(ind | (inv << 1)); a.ifr[p] = lf; a.ptRead[p] = r;
    }
    return;
  }
  const uint32_t n = a.c_count[c];
  const uint64_t src = a.c_start[c];
  const uint64_t g0 = g, pc0 = p;
  for (uint32_t i = lane; i < n; i += 64) {
    g = g0 + i; p = pc0 + 2 * (uint64_t)i + ((!a.single && i >= 1) ? 2 : 0);
    const uint32_t q = a.q[src + i], t = a.t[src + i];
    const int len = a.len[src + i];
    const uint32_t lf = (uint32_t)(g - f0);
    a.fq[g] = q; a.ft[g] = t; a.flen[g] = len; a.fcl[g] = cl; a.fai[g] = i;
    a.fval[g] = len * rate;                                            // Value[ii].val = matchesLengths * rate (:2206)
    a.fprevNode[g] = NONE; a.fprevInd[g] = NONE; a.fflags[g] = 3; a.used[g] = 0; a.fstrand[g] = (uint8_t)(strand != 0);
    const bool edge = !a.single && (i == 0 || i == n - 1);                 // the single-cluster SDP (SparseDP.h:2296-2305) inserts one pair only
    for (int rep = 0; rep < (edge ? 2 : 1); rep++) {
      const int pair = (strand == 0) ? rep : 1 - rep;                  // forward cluster: s1/e1 first; reverse: s2/e2 first
      uint32_t sq, st, eq, et;
      if (pair == 0) { sq = q; st = t; eq = q + len; et = t + len; }   // insertPointsPair :79-137
      else { sq = q; st = t + len; eq = q + len; et = t; }
      const uint8_t inv = pair == 0 ? 1 : 0;
      for (int e = 0; e < 2; e++, p++) {
        const uint32_t pq = e ? eq : sq, pt = e ? et : st;
        const uint8_t ind = e ? 0 : 1;
        a.key1[p] = ((uint64_t)pq << 33) | ((uint64_t)pt << 1) | ind; // SortByRowOp: q, t, ind (Sorting.h:226)
        a.pay1[p] = (uint32_t)(p - p0);
        a.iq[p] = pq; a.it[p] = pt; a.ifl[p] = (uint8_t)(ind | (inv << 1)); a.ifr[p] = lf; a.ptRead[p] = r;
      }
    }
  }
}

// after the row sort: gather the point attributes into H1 order, build the column-sort and diagonal-sort keys
__global__ void k_gather(uint64_t np, const uint32_t* __restrict__ ptRead, const uint64_t* __restrict__ ptOff, const uint32_t* __restrict__ pay1,
                         const uint32_t* __restrict__ iq, const uint32_t* __restrict__ it, const uint8_t* __restrict__ ifl,
                         const uint32_t* __restrict__ ifr, uint32_t* hq, uint32_t* ht, uint8_t* hfl, uint32_t* hfr, uint64_t* key2,
                         uint32_t* pay2, uint64_t* key3, uint32_t* pay3) {
  uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= np) return;
  const uint64_t p0 = ptOff[ptRead[p]];
  const uint64_t s = p0 + pay1[p];
  const uint32_t q = iq[s], t = it[s];
  const uint8_t fl = ifl[s];
  hq[p] = q; ht[p] = t; hfl[p] = fl; hfr[p] = ifr[s];
  key2[p] = ((uint64_t)t << 31) | ((uint64_t)q << 1) | (fl & 1);       // SortByColOp: t, q, ind (Sorting.h:241)
  pay2[p] = (uint32_t)(p - p0);
  const int inv = (fl >> 1) & 1, ind = fl & 1;
  const uint64_t cls = (uint64_t)((inv ? 0 : 2) + (ind ? 0 : 1));      // 0: s1, 1: e1, 2: s2, 3: e2
  const uint64_t dg = inv ? (uint64_t)((int64_t)t - (int64_t)q + (1LL << 32)) : (uint64_t)t + q;
  key3[p] = (cls << 40) | dg;
  pay3[p] = (uint32_t)(p - p0);
}

// before a read is re-run with larger stacks: Value[] back to its initial state (SparseDP.h:2206), status cleared
__global__ void k_reset_frags(int r0, const uint32_t* __restrict__ order, const uint64_t* __restrict__ fragOff, const int32_t* __restrict__ flen,
                              const float* __restrict__ rate_in, float rate, float* fval, uint32_t* fprevNode, uint32_t* fprevInd, uint8_t* fflags,
                              uint32_t* status) {
  const int r = r0 + (int)order[blockIdx.x];
  const float rt = rate_in ? rate_in[r] : rate;
  for (uint64_t g = fragOff[r] + threadIdx.x; g < fragOff[r + 1]; g += blockDim.x) { fval[g] = flen[g] * rt; fprevNode[g] = NONE; fprevInd[g] = NONE; fflags[g] = 3; }
  if (threadIdx.x == 0) status[r] = 0;
}

__global__ void k_pen_table(PwlTab pw, int n, short* tab, int* bad) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= n) return;
  const float w = pwl_w(pw.slope, pw.inter, pw.c1, pw.c2, 0, (long long)d);      // x = d + 1
  const float p = -w;                                                            // the penalty: an integer
  if (!(p >= 0.f && p <= 32767.f) || (float)(int)p != p) { atomicOr(bad, 1); tab[d] = 0; return; }
  tab[d] = (short)(int)p;
}

__global__ void k_frag_read(int n_reads, const uint64_t* __restrict__ fragOff, uint32_t* fragRead) {
  int r = blockIdx.x;
  for (uint64_t g = fragOff[r] + threadIdx.x; g < fragOff[r + 1]; g += blockDim.x) fragRead[g] = r;
}

inline dim3 grid256(uint64_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

namespace lra_sdp {

void launch_cluster_counts(hipStream_t st, uint64_t nc, const uint32_t* c_count, uint32_t* fragCnt, uint32_t* ptCnt, int single) {
  hipLaunchKernelGGL(k_cluster_counts, grid256(nc), dim3(256), 0, st, nc, c_count, fragCnt, ptCnt, single);
}
void launch_read_offsets(hipStream_t st, int n_reads, const uint64_t* cluster_off, const uint64_t* clusFragOff, const uint64_t* clusPtOff, uint64_t* fragOff, uint64_t* ptOff,
                         uint32_t* clusRead, uint32_t* status, uint32_t* nChains) {
  hipLaunchKernelGGL(k_read_offsets, grid256((uint64_t)n_reads + 1), dim3(256), 0, st, n_reads, cluster_off, clusFragOff, clusPtOff, fragOff, ptOff, clusRead, status, nChains);
}
void launch_points(hipStream_t st, const PtArgs& pa) {                 // box mode: a thread per cluster; anchor mode: a wave per cluster
  if (pa.qe) hipLaunchKernelGGL(k_points, dim3((unsigned)((pa.nc + 127) / 128)), dim3(128), 0, st, pa);
  else hipLaunchKernelGGL(k_points, dim3((unsigned)((pa.nc + 3) / 4)), dim3(256), 0, st, pa);
}
void launch_frag_read(hipStream_t st, int n_reads, const uint64_t* fragOff, uint32_t* fragRead) {
  hipLaunchKernelGGL(k_frag_read, dim3(n_reads), dim3(64), 0, st, n_reads, fragOff, fragRead);
}
void launch_gather(hipStream_t st, uint64_t np, const uint32_t* ptRead, const uint64_t* ptOff, const uint32_t* pay1, const uint32_t* iq, const uint32_t* it, const uint8_t* ifl,
                   const uint32_t* ifr, uint32_t* hq, uint32_t* ht, uint8_t* hfl, uint32_t* hfr, uint64_t* key2, uint32_t* pay2, uint64_t* key3, uint32_t* pay3) {
  hipLaunchKernelGGL(k_gather, grid256(np), dim3(256), 0, st, np, ptRead, ptOff, pay1, iq, it, ifl, ifr, hq, ht, hfl, hfr, key2, pay2, key3, pay3);
}
void launch_reset_frags(hipStream_t st, int n, int r0, const uint32_t* order, const uint64_t* fragOff, const int32_t* flen, const float* rate_in, float rate, float* fval,
                        uint32_t* fprevNode, uint32_t* fprevInd, uint8_t* fflags, uint32_t* status) {
  hipLaunchKernelGGL(k_reset_frags, dim3(n), dim3(64), 0, st, r0, order, fragOff, flen, rate_in, rate, fval, fprevNode, fprevInd, fflags, status);
}
void launch_pen_table(hipStream_t st, const PwlTab& pw, short* tab, int* bad) {
  hipLaunchKernelGGL(k_pen_table, dim3(PEN_TAB_WG / 256), dim3(256), 0, st, pw, PEN_TAB_WG, tab, bad);
}
void launch_arena_estimate(hipStream_t st, int n, int r0, const uint64_t* ptOff, float fE, float fN, uint32_t* cntE, uint32_t* cntN, uint32_t* cntD) {
  hipLaunchKernelGGL(k_arena_estimate, dim3((n + 255) / 256), dim3(256), 0, st, n, r0, ptOff, fE, fN, cntE, cntN, cntD);
}
void launch_arena_sizes(hipStream_t st, int n, int r0, const uint64_t* ptOff, const uint32_t* cntE, const uint32_t* cntN, const uint32_t* cntD, const uint32_t* lines, ReadArena* ra,
                        uint64_t* bytes, const uint32_t* order, int shift) {
  hipLaunchKernelGGL(k_arena_sizes, dim3((n + 255) / 256), dim3(256), 0, st, n, r0, ptOff, cntE, cntN, cntD, lines, ra, bytes, order, shift);
}
void launch_arena_bases(hipStream_t st, int n, const uint64_t* byteOff, ReadArena* ra, const uint32_t* order, char* arena) {
  hipLaunchKernelGGL(k_arena_bases, dim3((n + 255) / 256), dim3(256), 0, st, n, byteOff, ra, order, arena);
}
void launch_visit_clear(hipStream_t st, int n, const ReadArena* ra, const uint64_t* byteOff, const uint32_t* order) {
  hipLaunchKernelGGL(k_visit_clear, dim3(n), dim3(256), 0, st, ra, byteOff, order);
}
void launch_big_lines(hipStream_t st, int n, int r0, const uint32_t* order, const uint64_t* ptOff, const uint32_t* hq, const uint32_t* ht, const uint32_t* h2, uint32_t* maxLines,
                      uint32_t* lines) {
  hipLaunchKernelGGL(k_big_lines, dim3(n), dim3(256), 0, st, r0, order, ptOff, hq, ht, h2, maxLines, lines);
}

}  // namespace lra_sdp

// lra_amd/csrc/exact_sort.hip -- the library's exact sort of (64-bit key, 32-bit payload) lists: every list ends in the permutation libstdc++'s std::sort leaves with
// the reference's masked comparison (GenomeTuple::operator<, TupleOps.h:76: bit 63 is the strand flag), ties included.  gfx950 only.
//
// It is a2 of seeding (MapRead.h:185, sort(readmm): CompareLists depends on the permutation of equal keys), the sparse DP's point and value orders (sdp.hip) and
// RefineSpace's k-mer lists (refine_space.hip).  The libstdc++ text itself is std_sort.h; here are the kernels that run it -- a workgroup per list with the partition
// done level by level (sort_wg_kernel, three size classes), a lane per list behind them (sort_kernel) --, the launch sequence, and the radix path for lists whose keys
// are all different (lra_sort_mostly_unique_batch).
#include "common.h"
#include "kmer.h"
#include "std_sort.h"
#include <algorithm>

namespace {

constexpr int SORT_CAP = 9000;   // tuples per read the LDS sort holds (16 B each + tables <= 160 KiB)

struct MaskedLess {
  template <class V> __host__ __device__ __forceinline__ bool operator()(const V& a, const V& b) const { return (a.k & KM_FOR_MASK) < (b.k & KM_FOR_MASK); }
};

// std::sort on (key, pos) pairs, one lane per list: the lists beyond every workgroup mode (more than 2^26 tuples), flagged by the launches before it
__global__ void __launch_bounds__(64) sort_kernel(int n_reads, const uint64_t* __restrict__ mm_off, uint64_t* mm_key, uint32_t* mm_pos,
                                                  const int* __restrict__ only_flagged) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= n_reads) return;
  if (only_flagged && !only_flagged[r]) return;
  lra_std_sort::std_sort(lra_std_sort::Pairs<uint32_t>{mm_key + mm_off[r], mm_pos + mm_off[r]}, (long)(mm_off[r + 1] - mm_off[r]), MaskedLess());
}

// ---- the fast path: the same std::sort, one workgroup per list, data in LDS.
// Two facts make introsort data-parallel without changing its result:
//  (1) the segments the loop recurses into are disjoint, so they can be processed level by
//      level, all segments of a level at once;
//  (2) libstdc++'s unguarded Hoare partition of [first+1,last) around *first is a closed form:
//      with a_1<a_2<... the positions holding x >= pivot (ascending) and b_1>b_2>... those
//      holding x <= pivot (descending), it swaps (a_i,b_i) for i <= m = #{i: a_i < b_i} and
//      returns cut = min(a_{m+1}, b_m).  Ranks come from prefix counts, swaps are independent.
// The final insertion sort is stable, and the <=16-element leftovers are mutually ordered, so
// it equals __insertion_sort of every leftover block on its own.
constexpr int SORT_NT = 1024;
constexpr int SORT_NW = SORT_NT / 64;

// MODE 1 (BIG): the same algorithm for lists of up to 65534 tuples (beyond the LDS capacity; the value order of a large read's sparse-DP fragments, the point
// lists of a large read, the k-mer lists of a 30 kb gap): the element arrays live in a per-workgroup global scratch, only the segment tables stay in
// LDS; it takes the lists the LDS kernel flagged and clears the flag of those it sorted.
// MODE 2 (HUGE): lists beyond that (a 1 Mb assembly contig has ~180 k minimizers; one lane per list with the literal introsort took 19.9 of the 24.3 s of a
// 256-contig -CONTIG batch): 32-bit indices, the segment tables in the global scratch as well, the prefix counts as two 32-bit halves of a 64-bit word.
// MODE 1 also reports what it had to leave behind (stat[0] = the longest such list, stat[1] = how many), so that the host sizes MODE 2's scratch and
// launches it -- and the one-lane-per-list kernel behind it -- only when there is something to do.
template <int MODE> struct SortTypes { typedef unsigned short IT; typedef uint32_t TT; };
template <> struct SortTypes<2> { typedef uint32_t IT; typedef uint64_t TT; };
// bytes of per-workgroup global scratch for lists of up to cap tuples (MODE 1: elements only; MODE 2: elements + tables + start bits)
__host__ __device__ inline size_t sort_scratch_bytes(int mode, size_t cap) {
  const size_t isz = mode == 2 ? 4 : 2, maxseg = (cap / 16 + 8 + 1) & ~(size_t)1;
  size_t b = cap * 8 + 4 * cap * isz + 64;
  if (mode == 2) b += 10 * maxseg * isz + (cap / 32 + 2) * 4 + 64;
  return (b + 255) & ~(size_t)255;
}
template <int MODE>
__global__ void __launch_bounds__(SORT_NT) sort_wg_kernel(int n_reads, const uint64_t* __restrict__ mm_off, uint64_t* mm_key, uint32_t* mm_pos,
                                                        void* tscratch, int cap, int* __restrict__ fallback,
                                                        const int* __restrict__ only, char* gscr, int* stat, int minLen = 0) {
  constexpr bool BIG = MODE >= 1, HUGE = MODE == 2;
  typedef typename SortTypes<MODE>::IT IT;
  typedef typename SortTypes<MODE>::TT TT;
  constexpr IT S_NONE = (IT)~(IT)0;
  constexpr int HB = HUGE ? 32 : 16;                                      // bits per half of a prefix word
  constexpr TT HM = (TT)(((TT)1 << HB) - 1);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NT_ = (int)blockDim.x, NW_ = NT_ >> 6;                         // (1024 threads per list; 256 for the launch that takes the short lists four to a CU)
  const int maxseg = (cap / 16 + 8 + 1) & ~1;                            // even: the word array behind the ten tables stays 4-byte aligned
  char* ebase = BIG ? gscr + (size_t)blockIdx.x * sort_scratch_bytes(MODE, (size_t)cap) : smem;
  uint64_t* key = (uint64_t*)ebase;
  IT* idx = (IT*)(key + cap);
  IT* seg = idx + cap;
  IT* pa = seg + cap;
  IT* pb = pa + cap;
  IT* sF = HUGE ? pb + cap : BIG ? (IT*)smem : pb + cap;                  // segment tables (current)
  IT* sL = sF + maxseg;
  IT* sD = sL + maxseg;
  IT* nF = sD + maxseg;         // next level
  IT* nL = nF + maxseg;
  IT* nD = nL + maxseg;
  IT* sCut = nD + maxseg;
  IT* sLid = sCut + maxseg;
  IT* sRid = sLid + maxseg;
  IT* sM = sRid + maxseg;
  unsigned int* startBits = (unsigned int*)(sM + maxseg + (maxseg & 1));   // leftover-block start markers, cap/32+1 words
  __shared__ int cnt[4];                    // nseg, nnext
  __shared__ unsigned int waveTot[2 * SORT_NW];
  TT* t32 = (TT*)tscratch + (size_t)blockIdx.x * (size_t)(cap + 64);
  const lra_std_sort::Pairs<IT> S{key, idx};                              // (key, original index) pairs in LDS (or, for the larger modes, in the global scratch)
  const MaskedLess lt;
  for (int r = blockIdx.x; r < n_reads; r += gridDim.x) {
    const long base = (long)mm_off[r];
    const int n = (int)(mm_off[r + 1] - mm_off[r]);
    if (n < 2) continue;
    if (BIG) {
      if (!fallback[r]) continue;                                         // (every thread reads the flag before anyone clears it: the barrier below)
      if (n > cap) { if (MODE == 1 && stat && tid == 0) { atomicMax(&stat[0], n); atomicAdd(&stat[1], 1); } continue; }
    } else {
      if (only && !only[r]) continue;
      if (n < minLen) continue;                                           // (a shorter list was the previous launch's)
      if (n > cap) { if (fallback && tid == 0) { fallback[r] = 1; if (stat) atomicAdd(&stat[2], 1); } continue; }   // (stat[2]: lists left to the launch for large lists)
    }
    __syncthreads();
    if (BIG && tid == 0) fallback[r] = 0;
    for (int p = tid; p < n; p += NT_) { key[p] = mm_key[base + p]; idx[p] = (IT)p; seg[p] = 0; }
    for (int x = tid; x < cap / 32 + 1; x += NT_) startBits[x] = 0;
    if (tid == 0) {
      if (n > 16) { sF[0] = 0; sL[0] = (IT)n; sD[0] = (IT)(2 * (31 - __clz(n))); cnt[0] = 1; }
      else cnt[0] = 0;
      cnt[1] = 0;
    }
    __syncthreads();
    if (tid == 0) startBits[0] = 1u;
    int nseg = cnt[0];
    while (nseg > 0) {
      // (a) depth check / median of three -> pivot at `first`
      for (int s = tid; s < nseg; s += NT_) {
        const int first = (int)sF[s], last = (int)sL[s];
        sM[s] = 0;
        if (sD[s] == 0) { lra_std_sort::heap_sort(S, first, last, lt); sM[s] = S_NONE; continue; }
        sD[s] = sD[s] - 1;
        lra_std_sort::move_median_to_first(S, first, last, lt);
      }
      __syncthreads();
      // (b) exclusive prefix counts of the two stopper flags over all positions (wave w owns a
      //     contiguous range; ballots give in-row ranks)
      const int rows = (n + 63) / 64, rpw = (rows + NW_ - 1) / NW_;
      const int r0 = wave * rpw, r1 = min(rows, r0 + rpw);
      auto flags = [&](int p, bool& A, bool& B) {
        A = false; B = false;
        if (p < n) {
          const IT sg = seg[p];
          if (sg != S_NONE && sM[sg] != S_NONE && p != (int)sF[sg]) {
            const uint64_t piv = key[sF[sg]] & KM_FOR_MASK, km = key[p] & KM_FOR_MASK;
            A = km >= piv; B = km <= piv;
          }
        }
      };
      unsigned int totA = 0, totB = 0;
      for (int rw = r0; rw < r1; rw++) {
        bool A, B; flags(rw * 64 + lane, A, B);
        totA += __popcll(__ballot(A)); totB += __popcll(__ballot(B));
      }
      if (lane == 0) { waveTot[wave] = totA; waveTot[NW_ + wave] = totB; }
      __syncthreads();
      unsigned int baseA = 0, baseB = 0;
      for (int w = 0; w < wave; w++) { baseA += waveTot[w]; baseB += waveTot[NW_ + w]; }
      const unsigned long long below = (lane == 0) ? 0ULL : (~0ULL >> (64 - lane));
      for (int rw = r0; rw < r1; rw++) {
        const int p = rw * 64 + lane;
        bool A, B; flags(p, A, B);
        const unsigned long long mA = __ballot(A), mB = __ballot(B);
        if (p <= n) t32[p] = ((TT)(baseA + __popcll(mA & below)) & HM) | ((TT)(baseB + __popcll(mB & below)) << HB);
        baseA += __popcll(mA); baseB += __popcll(mB);
      }
      if (wave == NW_ - 1 && lane == 0 && (n & 63) == 0) t32[n] = ((TT)baseA & HM) | ((TT)baseB << HB);   // prefix at n when n is a row boundary
      __syncthreads();
      // (c) scatter stopper positions: pa ascending, pb descending, both stored from first+1
      for (int p = tid; p < n; p += NT_) {
        bool A, B; flags(p, A, B);
        if (A || B) {
          const int sg = (int)seg[p], b0 = (int)sF[sg] + 1;
          const TT t = t32[p], tb = t32[b0], te = t32[sL[sg]];
          if (A) pa[b0 + (int)(((t & HM) - (tb & HM)) & HM)] = (IT)p;
          if (B) pb[b0 + (int)(((te >> HB) - (t >> HB) - 1) & HM)] = (IT)p;
        }
      }
      __syncthreads();
      // (d) m = number of leading pairs with a_i < b_i
      for (int p = tid; p < n; p += NT_) {
        const IT sg = seg[p];
        if (sg == S_NONE || sM[sg] == S_NONE) continue;
        const int b0 = (int)sF[sg] + 1, i = p - b0;
        if (i < 0) continue;
        const TT tb = t32[b0], te = t32[sL[sg]];
        const int nA = (int)(((te & HM) - (tb & HM)) & HM), nB = (int)(((te >> HB) - (tb >> HB)) & HM);
        const int lim = min(nA, nB);
        if (i < lim && pa[b0 + i] < pb[b0 + i] && !(i + 1 < lim && pa[b0 + i + 1] < pb[b0 + i + 1])) sM[sg] = (IT)(i + 1);
      }
      __syncthreads();
      // (e) the swaps
      for (int p = tid; p < n; p += NT_) {
        const IT sg = seg[p];
        if (sg == S_NONE || sM[sg] == S_NONE) continue;
        const int b0 = (int)sF[sg] + 1, i = p - b0;
        if (i >= 0 && i < (int)sM[sg]) lra_std_sort::iter_swap(S, (int)pa[b0 + i], (int)pb[b0 + i]);
      }
      __syncthreads();
      // (f) cut -> children
      for (int s = tid; s < nseg; s += NT_) {
        const int first = (int)sF[s], last = (int)sL[s];
        if (sM[s] == S_NONE) { sCut[s] = (IT)last; sLid[s] = S_NONE; sRid[s] = S_NONE; continue; }   // heap sorted: finished
        const int b0 = first + 1, m = (int)sM[s];
        const TT tb = t32[b0], te = t32[last];
        const int nA = (int)(((te & HM) - (tb & HM)) & HM);
        int cut = 0x7fffffff;
        if (m < nA) cut = pa[b0 + m];
        if (m >= 1) cut = min(cut, (int)pb[b0 + m - 1]);
        sCut[s] = (IT)cut;
        IT lid = S_NONE, rid = S_NONE;
        if (cut - first > 16) { int x = atomicAdd(&cnt[1], 1); nF[x] = (IT)first; nL[x] = (IT)cut; nD[x] = sD[s]; lid = (IT)x; }
        if (last - cut > 16) { int x = atomicAdd(&cnt[1], 1); nF[x] = (IT)cut; nL[x] = (IT)last; nD[x] = sD[s]; rid = (IT)x; }
        atomicOr(&startBits[cut >> 5], 1u << (cut & 31));
        sLid[s] = lid; sRid[s] = rid;
      }
      __syncthreads();
      // (g) relabel elements, swap tables
      for (int p = tid; p < n; p += NT_) {
        const IT sg = seg[p];
        if (sg != S_NONE) seg[p] = (p < (int)sCut[sg]) ? sLid[sg] : sRid[sg];
      }
      nseg = cnt[1];
      __syncthreads();
      for (int s = tid; s < nseg; s += NT_) { sF[s] = nF[s]; sL[s] = nL[s]; sD[s] = nD[s]; }
      if (tid == 0) cnt[1] = 0;
      __syncthreads();
    }
    // final insertion sort of every leftover block (blocks start at the marked positions)
    for (int p = tid; p < n; p += NT_) {
      if ((startBits[p >> 5] >> (p & 31)) & 1u) {
        int q = p + 1;
        while (q < n && !((startBits[q >> 5] >> (q & 31)) & 1u)) q++;
        lra_std_sort::insertion_sort(S, p, q, lt);
      }
    }
    __syncthreads();
    uint32_t* tmp = HUGE ? (uint32_t*)seg : (uint32_t*)pa;            // pa|pb = 4*cap bytes (32-bit indices: seg, dead by now)
    for (int p = tid; p < n; p += NT_) tmp[p] = mm_pos[base + idx[p]];
    __syncthreads();
    for (int p = tid; p < n; p += NT_) { mm_key[base + p] = key[p]; mm_pos[base + p] = tmp[p]; }
  }
}

}  // namespace

int lra_sort_exact_batch(lra_ctx* ctx, int n_reads, const uint64_t* mm_off, uint64_t* mm_key, uint32_t* mm_pos, const lra_sort_opts& o, const int* only) {
  hipStream_t st = ctx->stream;
  const int nb = (n_reads + 63) / 64;
  const int cap = SORT_CAP, capB = 65534;                                 // unsigned short indices, 0xFFFF = none
  const int maxseg = (cap / 16 + 8 + 1) & ~1, maxsegB = (capB / 16 + 8 + 1) & ~1;
  const size_t lds = (size_t)cap * 16 + (size_t)maxseg * 20 + 8 + (size_t)(cap / 32 + 2) * 4;
  const size_t ldsB = (size_t)maxsegB * 20 + 8 + (size_t)(capB / 32 + 2) * 4 + 64;
  const int grid = n_reads < ctx->num_cu ? n_reads : ctx->num_cu;
  const int gridB = std::min(grid, 64);
  const size_t tszB = (size_t)gridB * (capB + 64) * 4, esz = (size_t)gridB * sort_scratch_bytes(1, (size_t)capB);
  uint32_t* tscr = (uint32_t*)lra_scratch(ctx, 0, (size_t)grid * (cap + 64) * 4 + (size_t)n_reads * 4);
  char* big = (char*)lra_ensure(ctx, 85, tszB + esz + 1024);               // its own buffer: callers hold pointers into scratch 0 across a sort
  int* stat = (int*)lra_ensure(ctx, 97, 64);                                 // slots 97 / 98 belong to the sort alone (86 / 87 hold fine_clusters.hip's results across sorts)
  if (!tscr || !big || !stat) return LRA_ERR_NOMEM;
  uint32_t* tscrB = (uint32_t*)big; char* gscr = big + tszB;
  int* flags = (int*)(tscr + (size_t)grid * (cap + 64));
  LRA_HIP_CHECK(ctx, hipMemsetAsync(flags, 0, (size_t)n_reads * 4, st));
  LRA_HIP_CHECK(ctx, hipMemsetAsync(stat, 0, 12, st));
  LRA_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)sort_wg_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  LRA_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)sort_wg_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsB));
  lra_time_begin(ctx, o.tag);
  // Lists of at most capS tuples first, 256 threads and ~36 KB of LDS each: four of them fit a CU where the 1024-thread / 156 KB launch holds one, and a short list's sort
  // is a chain of barriers either way (the sparse DP's value lists: hundreds of tuples, tens of thousands of lists).  Then the rest, as before.
  constexpr int capS = 2048;
  if (o.short_lists) {
    const int maxsegS = (capS / 16 + 8 + 1) & ~1;
    const size_t ldsS = (size_t)capS * 16 + (size_t)maxsegS * 20 + 8 + (size_t)(capS / 32 + 2) * 4;
    const int gridS = std::min(n_reads, std::min(ctx->num_cu * 4, (int)(((size_t)grid * (cap + 64)) / (size_t)(capS + 64))));
    hipLaunchKernelGGL(sort_wg_kernel<0>, dim3(gridS), dim3(256), ldsS, st, n_reads, mm_off, mm_key, mm_pos, (void*)tscr, capS, (int*)nullptr, only, (char*)nullptr, (int*)nullptr, 0);
  }
  hipLaunchKernelGGL(sort_wg_kernel<0>, dim3(grid), dim3(SORT_NT), lds, st, n_reads, mm_off, mm_key, mm_pos, (void*)tscr, cap, flags, only, (char*)nullptr, stat, o.short_lists ? capS + 1 : 0);
  lra_time_end(ctx);
  // the launch for lists beyond the LDS capacity (1024-thread workgroups again, 64 of them, each waiting for room beside another batch's half) only when the LDS launch left
  // a list behind: it says how many, and the round trip that asks takes the place of the one behind the large-list launch
  int h_left = 1;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&h_left, stat + 2, 4, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  if (h_left == 0) return LRA_OK;
  lra_time_begin(ctx, o.tag);
  hipLaunchKernelGGL(sort_wg_kernel<1>, dim3(gridB), dim3(SORT_NT), ldsB, st, n_reads, mm_off, mm_key, mm_pos, (void*)tscrB, capB, flags, only, gscr, stat);
  lra_time_end(ctx);
  // what is left: lists of more than 65534 tuples (the minimizers of a contig of several hundred kb) -- how long, how many
  int h_stat[2] = {0, 0};
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(h_stat, stat, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  if (h_stat[1] == 0) return LRA_OK;
  const int capH = std::min(h_stat[0] + 64, (1 << 26));                    // (a list beyond 2^26 tuples stays with the one-lane kernel)
  // (a workgroup per list beyond 65534 tuples, as many at a time as the device has CUs: a -CONTIG batch of 1024 contigs has 1024 such lists of ~180 k tuples, 7 MB of
  // scratch each; with a quarter of the CUs the launch took 370 ms)
  const int gridH = std::min(h_stat[1], std::max(1, ctx->num_cu));
  const size_t eszH = sort_scratch_bytes(2, (size_t)capH), tszH = (size_t)(capH + 64) * 8;
  char* huge = (char*)lra_ensure(ctx, 98, (size_t)gridH * (eszH + tszH) + 1024);
  if (!huge) return LRA_ERR_NOMEM;
  lra_time_begin(ctx, o.tag);
  hipLaunchKernelGGL(sort_wg_kernel<2>, dim3(gridH), dim3(SORT_NT), 0, st, n_reads, mm_off, mm_key, mm_pos, (void*)huge, capH, flags, only, huge + (size_t)gridH * tszH, (int*)nullptr);
  lra_time_end(ctx);
  if (h_stat[0] > capH) {
    lra_time_begin(ctx, o.fb_tag);
    hipLaunchKernelGGL(sort_kernel, dim3(nb), dim3(64), 0, st, n_reads, mm_off, mm_key, mm_pos, (const int*)flags);
    lra_time_end(ctx);
  }
  return LRA_OK;
}

// A list whose keys are all different has only one sorted order, so any sort reproduces std::sort on it.  Lists are radix-sorted into
// (tmp_key, tmp_pos); one block per list then looks for two equal neighbours: without any, the sorted list is copied over the input,
// with one the input is left alone and the list is marked for the exact sort.
__global__ void __launch_bounds__(256) sort_adopt_kernel(int n_lists, const uint64_t* __restrict__ off, uint64_t* key, uint32_t* pos,
                                                         const uint64_t* __restrict__ tkey, const uint32_t* __restrict__ tpos, int* ties, int* n_ties) {
  const int r = blockIdx.x;
  const uint64_t b = off[r], e = off[r + 1];
  int tie = 0;
  for (uint64_t i = b + threadIdx.x; i + 1 < e; i += 256) tie |= (tkey[i] & KM_FOR_MASK) == (tkey[i + 1] & KM_FOR_MASK);   // (what the exact sort's comparison sees: bit 63 is a flag)
  tie = __syncthreads_or(tie);
  if (tie) { if (threadIdx.x == 0) { ties[r] = 1; atomicAdd(n_ties, 1); } return; }
  if (threadIdx.x == 0) ties[r] = 0;
  for (uint64_t i = b + threadIdx.x; i < e; i += 256) { key[i] = tkey[i]; pos[i] = tpos[i]; }
}

// Same result as lra_sort_minimizers_batch, for keys that rarely repeat within a list (the sparse DP's point orders): keys below
// 2^end_bit, `total` = d_off[n_lists], (tmp_key, tmp_pos) = scratch of the same size as the input.
int lra_sort_mostly_unique_batch(lra_ctx* ctx, int n_lists, const uint64_t* d_off, uint64_t total, uint64_t* d_key, uint32_t* d_pos,
                                 uint64_t* tmp_key, uint32_t* tmp_pos, int end_bit, const lra_sort_opts& o) {
  if (n_lists == 0 || total == 0) return LRA_OK;
  hipStream_t st = ctx->stream;
  size_t temp_bytes = 0;
  (void)lra_segsort_pairs(ctx, nullptr, temp_bytes, nullptr, nullptr, nullptr, nullptr, (unsigned int)total, (unsigned int)n_lists, nullptr, nullptr, 0, end_bit, st);
  char* temp = (char*)lra_scratch(ctx, 2, temp_bytes + 512 + (size_t)n_lists * 4);
  if (!temp) return LRA_ERR_NOMEM;
  int* ties = (int*)(temp + ((temp_bytes + 255) & ~(size_t)255));
  int* n_ties = ties + n_lists + 1;
  LRA_HIP_CHECK(ctx, hipMemsetAsync(n_ties, 0, 4, st));
  lra_time_begin(ctx, o.tag);
  hipError_t e = lra_segsort_pairs(ctx, temp, temp_bytes, d_key, tmp_key, d_pos, tmp_pos, (unsigned int)total, (unsigned int)n_lists, d_off, d_off + 1, 0, end_bit, st);
  if (e != hipSuccess) { lra_time_end(ctx); return lra_set_err(ctx, LRA_ERR_HIP, "segmented sort: %s", hipGetErrorString(e)); }
  hipLaunchKernelGGL(sort_adopt_kernel, dim3(n_lists), dim3(256), 0, st, n_lists, d_off, d_key, d_pos, (const uint64_t*)tmp_key, (const uint32_t*)tmp_pos, ties, n_ties);
  lra_time_end(ctx);
  // Lists with a repeated key are rare in the sparse DP's point orders: without any, the exact sort's three launches -- workgroups that need a whole CU's LDS each, and wait
  // for it beside another batch's half -- and their closing round trip are left out (this round trip takes its place)
  int h_ties = 1;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&h_ties, n_ties, 4, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  if (h_ties == 0) return LRA_OK;
  // lra_scratch slot 0 is lra_sort_exact_batch's own; the ties mask lives in slot 2 and stays valid through it
  int rc = lra_sort_exact_batch(ctx, n_lists, d_off, d_key, d_pos, o, ties);
  if (rc) return rc;
  LRA_HIP_CHECK(ctx, hipGetLastError());
  return LRA_OK;
}

extern "C" int lra_sort_minimizers_batch(lra_ctx* ctx, int n_lists, const uint64_t* d_off, uint64_t* d_key, uint32_t* d_pos) {
  if (!ctx || n_lists < 0) return LRA_ERR_INVALID;
  if (n_lists == 0) return LRA_OK;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int rc = lra_sort_exact_batch(ctx, n_lists, d_off, d_key, d_pos);
  if (rc) return rc;
  LRA_HIP_CHECK(ctx, hipGetLastError());
  return LRA_OK;
}

// The host instantiation of what sort_kernel runs on the device
extern "C" int lra_sort_minimizers_host(uint64_t n, uint64_t* h_key, uint32_t* h_pos) {
  if (n && (!h_key || !h_pos)) return LRA_ERR_INVALID;
  lra_std_sort::std_sort(lra_std_sort::Pairs<uint32_t>{h_key, h_pos}, (long)n, MaskedLess());
  return LRA_OK;
}

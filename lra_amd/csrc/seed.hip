// lra_amd/csrc/seed.hip -- tier-1 seeding of a read batch on gfx950.
//
// Replaces, for a whole batch of reads resident in HBM, the first stages of MapRead
// (reference: MapRead.h:169-203):
//   a1  StoreMinimizers<GenomeTuple,Tuple>(read, globalK, globalW)        MinCount.h:8-179
//   a2  sort(readmm.begin(), readmm.end())                                MapRead.h:185 (the sort itself: exact_sort.hip)
//   a3  CompareLists<GenomeTuple,Tuple>(readmm, genomemm, allMatches)     CompareLists.h:9-146
//   a4  SeparateMatchesByStrand(read, genome, k, allMatches, for, rev)    MapRead.h:109-150
//
// Layout in HBM (structure of arrays, CSR by read):
//   reads    : uint8 seq[], uint64 read_off[n+1]
//   minimizers: uint64 mm_key[] (strand in bit 63, TupleOps.h:68), uint32 mm_pos[], uint64 mm_off[n+1]
//   index    : uint64 idx_key[] sorted by (key & 2^63-1), uint32 idx_pos[]   (the .mms payload, MMIndex.h:416)
//   matches  : uint32 match_qi[] (index into the read's sorted minimizers), uint32 match_ti[]
//              (index into the global index), uint64 match_off[n+1], in the reference's
//              discovery order; then per read forward-strand matches first, reverse after:
//              uint32 sep_qpos[], sep_tpos[], uint32 n_forward[n].
//
// Why these stages are emulated step by step instead of re-derived: their outputs depend
// on implementation details -- the unmasked first-window comparison and ring-index
// tie-break of the minimizer scan, the permutation libstdc++'s introsort leaves among
// equal keys (MapRead.h:185 sorts with a non-total order), and CompareLists' alternating
// two-ended walk with raw-key run skipping (which re-emits or drops pairs depending on
// that permutation).  Parallelism is across reads (one lane per read for the serial
// state machines) and across query tuples (one lane per tuple for the index searches,
// which are the HBM-heavy part).
#include "common.h"
#include <rocprim/rocprim.hpp>
#include "scan.h"

namespace {

constexpr uint64_t FOR_MASK = ~(1ULL << 63);  // lra.cpp:1008-1012
constexpr uint64_t REV_MASK = (1ULL << 63);
constexpr int MAX_W = 32;

__device__ __forceinline__ int code_n(unsigned char c) {  // SeqUtils.h:42 (seqMapN)
  if (c < 8) return c & 3;
  switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return 4;
  }
}
__device__ __forceinline__ uint64_t code2(unsigned char c) {  // SeqUtils.h:7 (seqMap)
  int v = code_n(c);
  return v > 3 ? 0 : (uint64_t)v;
}

// ------------------------------------------------------------------------------------ a1
// One lane per read; the state machine of MinCount.h:8-179 verbatim in behaviour.
// EMIT=false only counts.  The w-entry ring lives in LDS, lane-interleaved.  The reads are those of `list` (the reads with a non-ACGT byte, which the wave kernel
// below leaves to this one): the kernel is launched over them alone, and not at all when there are none.
template <bool EMIT>
__global__ void __launch_bounds__(64) sketch_kernel(int n_reads, const unsigned char* __restrict__ seq_all,
                                                    const uint64_t* __restrict__ read_off, int k, int w,
                                                    const uint64_t* __restrict__ mm_off, uint64_t* __restrict__ mm_key,
                                                    uint32_t* __restrict__ mm_pos, uint32_t* __restrict__ counts,
                                                    const int* __restrict__ list, int n_list) {
  __shared__ uint64_t ringT[MAX_W * 64];
  __shared__ uint32_t ringP[MAX_W * 64];
  const int lane = threadIdx.x;
  const int x = blockIdx.x * 64 + lane;
  if (x >= n_list) return;
  const int r = list[x];
  if (r < 0 || r >= n_reads) return;
  const unsigned char* seq = seq_all + read_off[r];
  const uint32_t seqLen = (uint32_t)(read_off[r + 1] - read_off[r]);
  uint64_t* okey = EMIT ? mm_key + mm_off[r] : nullptr;
  uint32_t* opos = EMIT ? mm_pos + mm_off[r] : nullptr;
  uint32_t n = 0;
#define SK_EMIT(T_, P_) do { if (EMIT) { okey[n] = (T_); opos[n] = (P_); } n++; } while (0)
#define SK_DONE() do { if (!EMIT) counts[r] = n; return; } while (0)
  const int span = w + k - 1;                                          // :17
  if (seqLen < (uint32_t)k || seqLen < (uint32_t)span) SK_DONE();      // :12,:26
  const uint64_t kmask = (k >= 32) ? ~0ULL : ((1ULL << (2 * k)) - 1);
  long nvStart = 0, nvEnd = 0;
  bool valid = false;
  auto find_valid = [&]() -> bool {                                    // :27-41 / :117-131
    valid = false;
    while ((uint32_t)nvStart < seqLen - (uint32_t)span && !valid) {
      valid = true;
      for (long x = nvStart; valid && x < nvStart + span; x++)
        if (code_n(seq[x]) > 3) { nvStart = x + 1; valid = false; }
    }
    return valid;
  };
  if (!find_valid()) SK_DONE();
  nvEnd = nvStart + span;
  uint64_t cur = 0, rc = 0;
  for (int p = 0; p < k; p++) cur = (cur << 2) + code2(seq[p]);        // StoreTuple TupleOps.h:104
  {
    uint64_t a = cur;                                                  // TupleRC TupleOps.h:125
    for (int i = 0; i < k; i++) { rc = (rc << 2) + ((~a) & 3ULL); a >>= 2; }
  }
  auto canon = [&]() -> uint64_t {
    return ((cur & FOR_MASK) < (rc & FOR_MASK)) ? (cur & FOR_MASK) : (rc | REV_MASK);
  };
  auto shift = [&](uint32_t at) {                                      // TupleOps.h:114-123
    uint64_t c = code2(seq[at]);
    cur = ((cur << 2) & kmask) + c;
    rc = (rc >> 2) + (((~c) & 3ULL) << (2 * ((uint64_t)k - 1)));
  };
  uint64_t actT = canon();
  uint32_t actP = 0;
  ringT[0 * 64 + lane] = actT; ringP[0 * 64 + lane] = 0;
  uint32_t p;
  const uint32_t nk = seqLen - k + 1;
  for (p = 1; p < (uint32_t)w && p < nk; p++) {                        // :77-96
    shift(p + k - 1);
    uint64_t c = canon();
    if (c < actT) { actT = c; actP = p; }                              // unmasked compare (:91)
    ringT[(p % w) * 64 + lane] = c; ringP[(p % w) * 64 + lane] = p;
  }
  if (nvEnd == span) SK_EMIT(actT, actP);                              // :100-102
  uint32_t slot = (uint32_t)w % (uint32_t)w;                           // p % w, advanced incrementally
  for (p = w; p < nk; p++) {                                           // :105-178
    if (nvEnd == (long)(p + k - 1)) {
      if (code_n(seq[p + k - 1]) <= 3) nvEnd++;
      else {
        nvStart = p + k;
        if (!find_valid()) SK_DONE();
        nvEnd = nvStart + span;
      }
    }
    shift(p + k - 1);
    uint64_t c = canon();
    ringT[slot * 64 + lane] = c; ringP[slot * 64 + lane] = p;
    if (++slot == (uint32_t)w) slot = 0;
    if (p - w >= actP) {                                               // :148-162 re-scan, ring order
      actT = ringT[lane]; actP = ringP[lane];
      for (int j = 1; j < w; j++) {
        uint64_t t = ringT[j * 64 + lane];
        if ((t & FOR_MASK) < (actT & FOR_MASK)) { actT = t; actP = ringP[j * 64 + lane]; }
      }
      if (nvEnd == (long)(p + k)) SK_EMIT(actT, actP);
    } else if ((c & FOR_MASK) < (actT & FOR_MASK)) {                   // :164-173
      actT = c; actP = p;
      if (nvEnd == (long)(p + k)) SK_EMIT(actT, actP);
    }
  }
  SK_DONE();
#undef SK_EMIT
#undef SK_DONE
}

// ---- a1, fast path: one WAVE per read (reads without non-ACGT bytes; the others are flagged
// for the serial kernel above).  64 positions per tile:
//   * 2-bit codes of the tile are packed with two ballots; every lane cuts its own k-mer out of
//     the packed words and derives forward / reverse-complement keys with bit tricks;
//   * the serial state of MinCount.h is only "which position is the active minimizer".  After
//     position 2w-1 the active one is always a minimum (by masked key) of the current window
//     (every element that entered after the first window was compared against it on entry), so
//       act(p) = p                      if key[p] <  min of the previous window
//              = ring-order argmin(p)   if act(p-1) just left the window      (:148-154)
//              = act(p-1)               otherwise,
//     and a tuple is emitted in the first two cases (:155-172).  Wherever the window minimum is
//     unique act(p) is that position regardless of history, so lanes resolve independently and
//     only lanes inside a run of tied minima are walked in order;
//   * positions below 2w (first window chosen with the UNMASKED comparison, :91) are replayed
//     literally by the whole wave on uniform values.
__device__ __forceinline__ uint64_t spread32(uint64_t x) {
  x = (x | (x << 16)) & 0x0000FFFF0000FFFFULL;
  x = (x | (x << 8)) & 0x00FF00FF00FF00FFULL;
  x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0FULL;
  x = (x | (x << 2)) & 0x3333333333333333ULL;
  x = (x | (x << 1)) & 0x5555555555555555ULL;
  return x;
}

// One pass: a read's minimizers are written where the read's bases begin in a staging array as long as the batch's bases (a read of L bases has at most L - k + 1
// of them), its count and whether it holds an N come out with them; sketch_compact moves the lists to their places once the counts are scanned.  (Two passes --
// count, scan, emit -- ran the whole window machine twice: 13.7 + 12.9 ms.)
template <bool EMIT>
__global__ void __launch_bounds__(64) sketch_wave_kernel(int n_reads, const unsigned char* __restrict__ seq_all,
                                                         const uint64_t* __restrict__ read_off, int k, int w,
                                                         const uint64_t* __restrict__ mm_off, uint64_t* __restrict__ mm_key,
                                                         uint32_t* __restrict__ mm_pos, uint32_t* __restrict__ counts, int* flagN,
                                                         int* __restrict__ n_flagged, int* __restrict__ flagged) {
  __shared__ uint64_t kbuf[128];
  const int lane = threadIdx.x;
  const uint64_t kbits = (k >= 32) ? 0xFFFFFFFFULL : ((1ULL << k) - 1);
  const uint64_t mask2k = (k >= 32) ? ~0ULL : ((1ULL << (2 * k)) - 1);
  const unsigned long long below = (lane == 0) ? 0ULL : (~0ULL >> (64 - lane));
  for (int r = blockIdx.x; r < n_reads; r += gridDim.x) {
    const unsigned char* seq = seq_all + read_off[r];
    const uint32_t seqLen = (uint32_t)(read_off[r + 1] - read_off[r]);
    uint64_t* okey = EMIT ? mm_key + mm_off[r] : nullptr;
    uint32_t* opos = EMIT ? mm_pos + mm_off[r] : nullptr;
    uint32_t nout = 0;
    const int span = w + k - 1;
    if (seqLen < (uint32_t)k || seqLen <= (uint32_t)span) { if (lane == 0) { counts[r] = 0; flagN[r] = 0; } continue; }   // :12,:26-27
    const uint32_t nk = seqLen - k + 1;
    const uint32_t P0 = min((uint32_t)(2 * w), nk);
    bool hasN = false;
    uint64_t carry_m = 0; uint32_t carry_act = 0;
    // the bases come in 64-byte pieces, one per tile, asked for two tiles ahead: piece j is tile j's own bases and (its first k - 1) the tail of tile j - 1's k-mers;
    // a tile's step is otherwise a chain that begins with a load from HBM and nothing to do until it is back
    unsigned char pc0 = lane < (int)seqLen ? seq[lane] : (unsigned char)'A', pc1 = 64u + lane < seqLen ? seq[64 + lane] : (unsigned char)'A';
    for (uint32_t B = 0; B < nk; B += 64) {
      // ---- keys of positions B..B+63
      const uint32_t p = B + lane;
      const unsigned char pn = p + 128 < seqLen ? seq[p + 128] : (unsigned char)'A';
      int c0 = 0, c1 = 0;
      if (p < seqLen) { int c = code_n(pc0); hasN |= c > 3; c0 = c & 3; }
      if (lane < k - 1 && p + 64 < seqLen) { int c = code_n(pc1); hasN |= c > 3; c1 = c > 3 ? 0 : c; }
      pc0 = pc1; pc1 = pn;
      const unsigned long long b0 = __ballot(c0 & 1), b1 = __ballot(c0 & 2), t0 = __ballot(c1 & 1), t1 = __ballot(c1 & 2);
      uint64_t x0 = b0 >> lane, x1 = b1 >> lane;
      if (lane) { x0 |= t0 << (64 - lane); x1 |= t1 << (64 - lane); }
      x0 &= kbits; x1 &= kbits;
      const uint64_t LE = spread32(x0) | (spread32(x1) << 1);
      const uint64_t rc = (~LE) & mask2k;
      uint64_t v = __brevll(LE);
      v = ((v >> 1) & 0x5555555555555555ULL) | ((v & 0x5555555555555555ULL) << 1);
      const uint64_t fwd = (k >= 32) ? v : (v >> (64 - 2 * k));
      const uint64_t key = ((fwd & FOR_MASK) < (rc & FOR_MASK)) ? (fwd & FOR_MASK) : (rc | REV_MASK);   // :60-61
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      kbuf[p & 127] = key;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      if (B == 0) {
        // ---- literal replay of positions 0..P0-1 on uniform values (all lanes identical)
        uint64_t actT = kbuf[0]; uint32_t actP = 0;
        for (uint32_t q = 1; q < (uint32_t)w && q < nk; q++) { uint64_t c = kbuf[q]; if (c < actT) { actT = c; actP = q; } }   // :77-96
        if (lane == 0 && EMIT) { okey[nout] = actT; opos[nout] = actP; }                                                       // :100-102
        nout++;
        for (uint32_t q = w; q < P0; q++) {                                                                                  // :105-178
          const uint64_t c = kbuf[q];
          bool em = false;
          if (q - w >= actP) {
            // ring slot j holds the newest position == j (mod w)
            uint64_t bt = 0; uint32_t bp = 0;
            for (int j = 0; j < w; j++) {
              uint32_t x = q - ((q - (uint32_t)j) % (uint32_t)w);
              uint64_t t = kbuf[x];
              if (j == 0 || (t & FOR_MASK) < (bt & FOR_MASK)) { bt = t; bp = x; }
            }
            actT = bt; actP = bp; em = true;
          } else if ((c & FOR_MASK) < (actT & FOR_MASK)) { actT = c; actP = q; em = true; }
          if (em) { if (lane == 0 && EMIT) { okey[nout] = actT; opos[nout] = actP; } nout++; }
        }
        carry_m = actT & FOR_MASK; carry_act = actP;
      }
      // ---- positions >= P0 of this tile, in parallel
      const bool live = p >= P0 && p < nk;
      uint64_t bk = key & FOR_MASK; uint32_t bpos = p; int br = (int)(p % (uint32_t)w), cnt = 1;
      if (live) {
        int rx = br;
        for (int d = 1; d < w; d++) {
          rx = (rx == 0) ? w - 1 : rx - 1;
          const uint32_t x = p - d;
          const uint64_t kx = kbuf[x & 127] & FOR_MASK;
          if (kx < bk) { bk = kx; bpos = x; br = rx; cnt = 1; }
          else if (kx == bk) { cnt++; if (rx < br) { br = rx; bpos = x; } }
        }
      }
      // min of the previous window = lane-1's window min (lane 0: carried over)
      uint64_t mprev = __shfl_up(bk, 1);
      const bool prevLive = lane > 0 && (p - 1) >= P0;
      if (!prevLive) mprev = carry_m;           // first live lane of the read, or lane 0 of a later tile
      const bool strictNew = live && (key & FOR_MASK) < mprev;
      uint32_t A = (cnt == 1 || strictNew) ? (strictNew ? p : bpos) : 0xFFFFFFFFu;
      // resolve lanes whose window minimum is tied, in order
      unsigned long long unk = __ballot(live && A == 0xFFFFFFFFu);
      while (unk) {
        const int l = __ffsll((long long)unk) - 1;
        unk &= unk - 1;
        uint32_t pa = __shfl(A, (l + 63) & 63);
        const uint32_t pl = B + l;
        if (l == 0 || pl - 1 < P0) pa = carry_act;
        const uint32_t posR = __shfl(bpos, l);
        const uint32_t a = (pa == pl - w) ? posR : pa;
        if (lane == l) A = a;
      }
      uint32_t prevA = __shfl_up(A, 1);
      if (!prevLive) prevA = carry_act;
      const bool em = live && (prevA == p - (uint32_t)w || strictNew);
      const unsigned long long me = __ballot(em);
      if (EMIT && em) {
        const uint32_t o = nout + __popcll(me & below);
        okey[o] = kbuf[A & 127]; opos[o] = A;
      }
      nout += __popcll(me);
      // carries: state after the last live position of this tile
      const unsigned long long ml = __ballot(live);
      if (ml) {
        const int last = 63 - __clzll((long long)ml);
        carry_m = __shfl(bk, last); carry_act = __shfl(A, last);
      }
      __builtin_amdgcn_wave_barrier();
    }
    const bool anyN = __ballot(hasN) != 0;
    if (lane == 0) {
      counts[r] = anyN ? 0 : nout;                                     // (a flagged read's count comes from the serial kernel, after the first scan)
      flagN[r] = anyN ? 1 : 0;
      if (anyN) flagged[atomicAdd(n_flagged, 1)] = r;                  // in any order: every read's tuples go to the read's own places
    }
  }
}

// the lists from the staging array (at the reads' base offsets) to their places; a read with an N is left to sketch_kernel
__global__ void __launch_bounds__(256) sketch_compact(int n_reads, const uint64_t* __restrict__ read_off, const uint64_t* __restrict__ mm_off, const int* __restrict__ flagN,
                                                      const uint64_t* __restrict__ wkey, const uint32_t* __restrict__ wpos, uint64_t* __restrict__ mm_key,
                                                      uint32_t* __restrict__ mm_pos) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int r = blockIdx.x * 4 + wv; r < n_reads; r += gridDim.x * 4) {
    if (flagN[r]) continue;
    const uint64_t src = read_off[r], dst = mm_off[r];
    const uint32_t n = (uint32_t)(mm_off[r + 1] - dst);
    for (uint32_t i = lane; i < n; i += 64) { mm_key[dst + i] = wkey[src + i]; mm_pos[dst + i] = wpos[src + i]; }
  }
}

// ---- a1 at w = 1 (lra align -a: StoreMinimizers(read, globalK, 1), MapRead.h:172-183).  With a window of one k-mer there is no window machine: MinCount.h:8-179
// emits, for a read of L > k bases, every position p < L - k whose k-mer holds no non-ACGT byte, and p = L - k only when that k-mer is clean AND seq[L - k - 1]
// is ACGT (both N searches, :27 and :115, stop before a window that starts at L - k, so the last k-mer is reached only by continuity); nothing when L <= k.
// Whether p is emitted depends on the bytes near p alone, so the stage is position-parallel over the batch's bases: tile t = positions
// [base + 64 t, base + 64 t + 64) of the concatenated reads (base = read_off[0]), reads of any length and reads with N alike.  Each wave takes a run of
// consecutive tiles and keeps the read it is in from one tile to the next; lanes of a tile that crosses a read boundary look their read up themselves.
// COUNT: tile_cnt[t] = emitted positions in tile t, tile_mask[t] = which.  EMIT: keys and positions straight to their final places, tile_pre[t] (the exclusive
// scan of tile_cnt) + the emitted lanes below.
__device__ __forceinline__ int read_at(const uint64_t* __restrict__ off, int lo, int hi, uint64_t g) {   // the last r in [lo, hi) with off[r] <= g (off[lo] <= g)
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off[mid] <= g) lo = mid; else hi = mid; }
  return lo;
}
constexpr int SKA_NT = 256;          // 4 waves per workgroup, each with its own run of tiles
template <bool EMIT>
__global__ void __launch_bounds__(SKA_NT) sketch_all_kernel(uint64_t n_tiles, uint64_t tiles_per_wave, int n_reads, const unsigned char* __restrict__ seq,
                                                            const uint64_t* __restrict__ read_off, int k, uint32_t* __restrict__ tile_cnt,
                                                            uint64_t* __restrict__ tile_mask, const uint64_t* __restrict__ tile_pre,
                                                            uint64_t* __restrict__ mm_key, uint32_t* __restrict__ mm_pos) {
  const int lane = threadIdx.x & 63;
  const uint64_t wave = (uint64_t)blockIdx.x * (SKA_NT / 64) + (threadIdx.x >> 6);
  const uint64_t t0 = wave * tiles_per_wave;
  if (t0 >= n_tiles) return;
  const uint64_t t1 = min(n_tiles, t0 + tiles_per_wave);
  const uint64_t base = read_off[0], end = read_off[n_reads];
  const uint64_t kbits = (k >= 32) ? 0xFFFFFFFFULL : ((1ULL << k) - 1);
  const uint64_t mask2k = (k >= 32) ? ~0ULL : ((1ULL << (2 * k)) - 1);
  const unsigned long long below = (lane == 0) ? 0ULL : (~0ULL >> (64 - lane));
  int r0 = read_at(read_off, 0, n_reads, base + t0 * 64);          // the read of the tile's first position (wave-uniform)
  uint64_t r0_end = read_off[r0 + 1];
  for (uint64_t t = t0; t < t1; t++) {
    const uint64_t G = base + t * 64, g = G + lane;
    if (G >= r0_end) { r0 = read_at(read_off, r0, n_reads, G); r0_end = read_off[r0 + 1]; }
    int r = r0; uint64_t rs = read_off[r0], re = r0_end;
    if (g >= r0_end && g < end) { r = read_at(read_off, r0, n_reads, g); rs = read_off[r]; re = read_off[r + 1]; }
    // this lane's byte and, for lanes below k - 1, one of the k - 1 bytes behind the tile (bytes past the batch read as 'A': no position there is emitted)
    const int cA = g < end ? code_n(seq[g]) : 0;
    const int cB = (lane < k - 1 && G + 64 + lane < end) ? code_n(seq[G + 64 + lane]) : 0;
    const unsigned long long nA = __ballot(cA > 3), nB = __ballot(cB > 3);
    uint64_t xn = nA >> lane;
    if (lane) xn |= nB << (64 - lane);
    const uint64_t L = re - rs, p = g - rs;
    bool em = g < end && L > (uint64_t)k && p <= L - k && (xn & kbits) == 0;
    if (em && p == L - k) em = code_n(seq[g - 1]) <= 3;              // the last k-mer: only after an ACGT byte (see above)
    const unsigned long long me = __ballot(em);
    if (!EMIT) {
      if (lane == 0) { tile_cnt[t] = (uint32_t)__popcll(me); tile_mask[t] = me; }
      continue;
    }
    if (!me) continue;
    // 2-bit codes packed by ballot, every lane cuts its own k-mer out (as sketch_wave_kernel; an N's code there is 0, it is never in an emitted k-mer)
    const int c0 = cA & 3, c1 = cB > 3 ? 0 : cB;
    const unsigned long long b0 = __ballot(c0 & 1), b1 = __ballot(c0 & 2), u0 = __ballot(c1 & 1), u1 = __ballot(c1 & 2);
    uint64_t x0 = b0 >> lane, x1 = b1 >> lane;
    if (lane) { x0 |= u0 << (64 - lane); x1 |= u1 << (64 - lane); }
    x0 &= kbits; x1 &= kbits;
    const uint64_t LE = spread32(x0) | (spread32(x1) << 1);
    const uint64_t rc = (~LE) & mask2k;
    uint64_t v = __brevll(LE);
    v = ((v >> 1) & 0x5555555555555555ULL) | ((v & 0x5555555555555555ULL) << 1);
    const uint64_t fwd = (k >= 32) ? v : (v >> (64 - 2 * k));
    if (em) {
      const uint64_t o = tile_pre[t] + (uint64_t)__popcll(me & below);
      mm_key[o] = ((fwd & FOR_MASK) < (rc & FOR_MASK)) ? (fwd & FOR_MASK) : (rc | REV_MASK);   // MinCount.h:60-61
      mm_pos[o] = (uint32_t)p;
    }
  }
}

// mm_off[r] = the emitted positions in front of read r's first base: tile_pre of its tile + the emitted lanes of that tile below it
__global__ void __launch_bounds__(256) sketch_all_offsets(int n_reads, const uint64_t* __restrict__ read_off, uint64_t n_tiles, const uint64_t* __restrict__ tile_pre,
                                                          const uint64_t* __restrict__ tile_mask, uint64_t* __restrict__ mm_off) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r > n_reads) return;
  const uint64_t d = read_off[r] - read_off[0], t = d >> 6;
  const int l = (int)(d & 63);
  mm_off[r] = t >= n_tiles ? tile_pre[n_tiles] : tile_pre[t] + (uint64_t)__popcll(tile_mask[t] & (l ? (~0ULL >> (64 - l)) : 0ULL));
}

// ------------------------------------------------------------------------------------ a3
// (i) per query tuple: global lower/upper bound of its masked key in the index.  Because the
// index is sorted by masked key, lower_bound over any sub-range [ts,te) is the global bound
// clamped to [ts,te] -- so the serial walk of CompareLists needs no searches of its own.
// A bucket directory over the top bits of the masked key (built once at index load) confines each
// search to a handful of entries: dir[b] = first index whose (key >> shift) >= b.
__global__ void dir_build_kernel(uint32_t nbuckets, int shift, const uint64_t* __restrict__ idx_key, uint64_t n_idx, uint32_t* __restrict__ dir) {
  uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b > nbuckets) return;
  if (b == nbuckets) { dir[b] = (uint32_t)n_idx; return; }
  const uint64_t q = b << shift;
  uint64_t lo = 0, hi = n_idx;
  while (lo < hi) { uint64_t mid = lo + ((hi - lo) >> 1); if ((idx_key[mid] & FOR_MASK) < q) lo = mid + 1; else hi = mid; }
  dir[b] = (uint32_t)lo;
}

// Also hands the walk the index keys it will look at when it lands on these bounds (T[lb], T[lb-1],
// T[ub-1]), so the serial walk itself makes no dependent loads from the index.
__global__ void bounds_kernel(uint64_t total, const uint64_t* __restrict__ mm_key, const uint64_t* __restrict__ idx_key,
                              uint64_t n_idx, const uint32_t* __restrict__ dir, uint32_t nbuckets, int shift,
                              uint32_t* __restrict__ lb, uint32_t* __restrict__ ub, uint64_t* __restrict__ tk_lb,
                              uint64_t* __restrict__ tk_lbm1, uint64_t* __restrict__ tk_ubm1) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const uint64_t q = mm_key[i] & FOR_MASK;
  uint64_t bkt = q >> shift;
  if (bkt >= nbuckets) bkt = nbuckets - 1;
  uint64_t lo = dir[bkt], hi = dir[bkt + 1];
  if (bkt == nbuckets - 1) hi = n_idx;
  const uint64_t hi0 = hi;
  while (lo < hi) { uint64_t mid = lo + ((hi - lo) >> 1); if ((idx_key[mid] & FOR_MASK) < q) lo = mid + 1; else hi = mid; }
  const uint64_t l = lo;
  // the end of the equal run: it starts at l and is short (most index keys occur once), so a few forward steps replace the second binary search from scratch
  // (the kernel is bandwidth-bound: every probe of a 1.5 GB key array is a cache line); a long run finishes with the search on what is left
  hi = hi0;
  { int steps = 0; while (lo < hi && steps < 4 && (idx_key[lo] & FOR_MASK) == q) { lo++; steps++; }
    if (steps == 4) { while (lo < hi) { uint64_t mid = lo + ((hi - lo) >> 1); if (!(q < (idx_key[mid] & FOR_MASK))) lo = mid + 1; else hi = mid; } } }
  const uint64_t u = lo;
  lb[i] = (uint32_t)l; ub[i] = (uint32_t)u;
  tk_lb[i] = (l < n_idx) ? idx_key[l] : 0;
  tk_lbm1[i] = (l > 0) ? idx_key[l - 1] : 0;
  tk_ubm1[i] = (u > 0) ? idx_key[u - 1] : 0;
}

// per-read upper bound on emitted pairs: a (query tuple, index tuple) pair with equal keys can be
// emitted by a front step, re-emitted once by the raw-key quirk (:101-102), and once by a back step
// opts.defer_seed_matches (scheduling only): the reads whose walk found more matches than T keep none of them -- every later stage sees a read without matches -- and are
// flagged; the driver marks them LRA_ST_DEFERRED and the caller maps them in a later batch of their own kind
__global__ void defer_heavy_kernel(int n_reads, uint32_t T, uint64_t* __restrict__ counts, uint8_t* __restrict__ flag) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_reads) return;
  const bool d = counts[r] > (uint64_t)T;
  flag[r] = d ? 1 : 0;
  if (d) counts[r] = 0;
}
__global__ void __launch_bounds__(64) match_capacity_kernel(int n_reads, const uint64_t* __restrict__ mm_off, const uint32_t* __restrict__ lb,
                                                            const uint32_t* __restrict__ ub, uint64_t* __restrict__ cap) {
  const int lane = threadIdx.x;
  for (int r = blockIdx.x; r < n_reads; r += gridDim.x) {
    uint64_t sum = 0;
    for (uint64_t i = mm_off[r] + lane; i < mm_off[r + 1]; i += 64) sum += (uint64_t)(ub[i] - lb[i]);
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if (lane == 0) cap[r] = 3 * sum;
  }
}

// (ii) the alternating two-ended walk of CompareLists.h:43-143, one lane per read.  T[ts] and
// T[te-1] live in registers and are refreshed from the prefetched neighbourhood arrays whenever
// ts / te jump to a bound; only the raw-key run skip (:101) still reads the index itself.
__global__ void __launch_bounds__(64) compare_kernel(int FLAT_LANES, int n_reads, const uint64_t* __restrict__ mm_off, const uint64_t* __restrict__ mm_key,
                                                     const uint32_t* __restrict__ lbA, const uint32_t* __restrict__ ubA,
                                                     const uint64_t* __restrict__ tkLbA, const uint64_t* __restrict__ tkLbm1A,
                                                     const uint64_t* __restrict__ tkUbm1A,
                                                     const uint64_t* __restrict__ idx_key, long n_idx, long maxFreq,
                                                     const uint64_t* __restrict__ match_off, uint32_t* __restrict__ match_qi,
                                                     uint32_t* __restrict__ match_ti, uint64_t* __restrict__ counts) {
  if (threadIdx.x >= FLAT_LANES) return;                                 // the walks of a wave's reads diverge: 32 reads per wave measured best (16: 39 ms, 32: 37, 64: 45)
  const int r = blockIdx.x * FLAT_LANES + threadIdx.x;
  if (r >= n_reads) return;
  const uint64_t* qk = mm_key + mm_off[r];
  const uint32_t* LB = lbA + mm_off[r];
  const uint32_t* UB = ubA + mm_off[r];
  const uint64_t* TKLB = tkLbA + mm_off[r];
  const uint64_t* TKLBM1 = tkLbm1A + mm_off[r];
  const uint64_t* TKUBM1 = tkUbm1A + mm_off[r];
  // (32-bit cursors: a read's tuples and the index both stay below 2^32 -- lb / ub are 32-bit -- and the walk is bound by instruction issue, where every 64-bit
  // compare or add is two)
  const int nq = (int)(mm_off[r + 1] - mm_off[r]);
  const uint32_t nt = (uint32_t)n_idx;
  const int mf = maxFreq > 0x7fffffffL ? 0x7fffffff : (int)maxFreq;
  uint32_t* oq = match_qi + match_off[r];
  uint32_t* ot = match_ti + match_off[r];
  const uint64_t room = match_off[r + 1] - match_off[r];
  uint64_t n = 0;
  const uint64_t M = FOR_MASK;
  if (nq != 0 && nt != 0) {                                            // :27-30
    int qs = 0, qe = nq - 1; uint32_t ts = 0, te = nt;
    uint64_t Tts = idx_key[0], Tte1 = idx_key[nt - 1];                 // raw T[ts], T[te-1]
    do {
      // Every load of a step depends on qs / qe only, which are known here: the step's tuples (three keys from each end, the bounds and index keys of qs and qe)
      // are asked for in one go -- one memory round trip per step instead of one per basic block (~6) -- and the loops below fall back to loads beyond them.
      const int pq = qs, eq = qe;
      const uint64_t pK0 = qk[pq], pK1 = qk[pq + 1 < nq ? pq + 1 : pq], pK2 = qk[pq + 2 < nq ? pq + 2 : pq];
      const uint32_t pLB = LB[pq], pUB = UB[pq]; const uint64_t pTL = TKLB[pq];
      const uint64_t eK0 = qk[eq], eK1 = qk[eq >= 1 ? eq - 1 : eq], eK2 = qk[eq >= 2 ? eq - 2 : eq];
      const uint32_t eLB = LB[eq], eUB = UB[eq]; const uint64_t eTU1 = TKUBM1[eq], eTL1 = TKLBM1[eq];
      auto QF = [&](int i) -> uint64_t { const int d = i - pq; return d == 0 ? pK0 : d == 1 ? pK1 : d == 2 ? pK2 : qk[i]; };   // raw key of tuple i, front / back
      auto QB = [&](int i) -> uint64_t { const int d = eq - i; return d == 0 ? eK0 : d == 1 ? eK1 : d == 2 ? eK2 : qk[i]; };
      while (qs <= qe && (QF(qs) & M) < (Tts & M)) qs++;               // :47-49
      if (qs >= qe) break;                                             // :51-53
      const uint64_t Qs = QF(qs) & M;
      uint64_t startGap = Qs - (Tts & M);
      while (qe > qs && te > ts && (QB(qe) & M) > (Tte1 & M)) qe--;    // :63-65
      const uint64_t Qe = QB(qe) & M;
      uint64_t endGap = (Tte1 & M) - Qe;
      if (startGap == 0 || (startGap & M) > (endGap & M)) {            // :69
        const uint32_t tsOrig = ts; const int qsOrig = qs;
        const uint64_t rawOrig = Tts;
        const uint32_t lo = qs == pq ? pLB : LB[qs];                   // lower_bound on [ts,te)  (:76)
        if (lo > ts) {
          if (lo >= te) ts = te;
          else { ts = lo; Tts = (qs == pq ? pTL : TKLB[qs]); }
        }
        if (ts < te && (Tts & M) == Qs) {
          const uint32_t tsStart = ts;
          uint32_t tsi = ts;
          { uint32_t e = qs == pq ? pUB : UB[qs]; e = e > te ? te : e; if (e > tsi) tsi = e; }   // end of the equal run inside [ts,te)
          const uint32_t qsStart = (uint32_t)qs;
          while (qs < qe && (QF(qs + 1) & M) == Qs) qs++;
          if (qs - (int)qsStart < mf) {
            for (uint32_t ti = tsStart; ti != tsi; ti++)
              for (uint32_t qi = qsStart; qi <= (uint32_t)qs; qi++) {
                if (n < room) { oq[n] = qi; ot[n] = ti; }
                n++;
              }
          }
        }
        if (ts == tsOrig) {                                            // :101 (a jump lands on a different key: no skip)
          while (ts < te && Tts == rawOrig) { ts++; if (ts < nt) Tts = idx_key[ts]; }
        }
        { const uint64_t raw = QF(qsOrig); while (qs < qe && QF(qs) == raw) qs++; }             // :102
      } else {
        if (te != nt && (Tte1 & M) == Qe) {                            // :112-114
        } else {                                                       // upper_bound on [ts,te) (:116-118)
          const uint32_t hi = qe == eq ? eUB : UB[qe];
          if (hi < te) {
            if (hi <= ts) te = ts;
            else { te = hi; Tte1 = (qe == eq ? eTU1 : TKUBM1[qe]); }
          }
        }
        const uint32_t teStart = te;
        uint32_t tei = te;
        if (tei > ts && (Tte1 & M) == Qe) {                      // start of the equal run inside [ts,te)
          const uint32_t b = qe == eq ? eLB : LB[qe];
          if (b <= ts) tei = ts;
          else { tei = b; Tte1 = (qe == eq ? eTL1 : TKLBM1[qe]); }
        }
        if (tei < teStart && teStart > 0) {
          const uint32_t qeStart = (uint32_t)qe;
          while (qe > qs && (QB(qe) & M) == (QB(qe - 1) & M)) qe--;
          if ((int)qeStart - qe < mf) {
            for (uint32_t ti = tei; ti < teStart; ti++)
              for (uint32_t qi = (uint32_t)qe; qi <= qeStart; qi++) {
                if (n < room) { oq[n] = qi; ot[n] = ti; }
                n++;
              }
          }
        }
        te = tei;
      }
    } while (qs < qe && ts < te);
  }
  counts[r] = n;
}

// ------------------------------------------------------------------------------------ a4
// One wave per read: strand flag per match (k-byte compare of read vs genome), then a stable
// partition (forward first) with ballot/popcount prefix sums.
__global__ void __launch_bounds__(64) strand_kernel(int n_reads, const unsigned char* __restrict__ seq_all, const uint64_t* __restrict__ read_off,
                                                    const unsigned char* __restrict__ genome, int k,
                                                    const uint64_t* __restrict__ mm_off, const uint32_t* __restrict__ mm_pos,
                                                    const uint32_t* __restrict__ idx_pos,
                                                    const uint64_t* __restrict__ match_off, const uint64_t* __restrict__ src_off,
                                                    const uint32_t* __restrict__ src_qi, const uint32_t* __restrict__ src_ti,
                                                    uint32_t* __restrict__ match_qi, uint32_t* __restrict__ match_ti, uint32_t* __restrict__ sep_qpos,
                                                    uint32_t* __restrict__ sep_tpos, uint32_t* __restrict__ n_forward,
                                                    const uint64_t* __restrict__ mm_key, uint64_t* __restrict__ sep_qkey) {
  const int lane = threadIdx.x;
  for (int r = blockIdx.x; r < n_reads; r += gridDim.x) {
    const unsigned char* read = seq_all + read_off[r];
    const uint32_t* qpos_of = mm_pos + mm_off[r];
    const uint64_t m0 = match_off[r], m1 = match_off[r + 1];
    // pass 0: compact the pairs out of the capacity-spaced walk buffer
    for (uint64_t i = m0 + lane; i < m1; i += 64) { match_qi[i] = src_qi[src_off[r] + (i - m0)]; match_ti[i] = src_ti[src_off[r] + (i - m0)]; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    // pass 1: count forward matches
    uint64_t nf = 0;
    for (uint64_t base = m0; base < m1; base += 64) {
      uint64_t i = base + lane;
      bool fwd = false;
      if (i < m1) {
        const unsigned char* a = read + qpos_of[match_qi[i]];
        const unsigned char* b = genome + idx_pos[match_ti[i]];
        // (k bytes of each side, eight at a time and all asked for at once: a byte loop with an early exit is k round trips in a row)
        fwd = true;
        int x = 0;
        for (; x + 8 <= k; x += 8) { unsigned long long wa, wb; __builtin_memcpy(&wa, a + x, 8); __builtin_memcpy(&wb, b + x, 8); fwd = fwd && wa == wb; }
        for (; x < k; x++) fwd = fwd && a[x] == b[x];
        if (fwd) match_qi[i] |= 0x80000000u;                               // remembered for pass 2 (the same lane reads it back): the k-byte compare costs two cache
      }                                                                    // lines of random access per match -- 12 GB per batch -- and was made twice
      nf += __popcll(__ballot(fwd));
    }
    if (lane == 0) n_forward[r] = (uint32_t)nf;
    // pass 2: stable partition
    uint64_t fcur = m0, rcur = m0 + nf;
    for (uint64_t base = m0; base < m1; base += 64) {
      uint64_t i = base + lane;
      bool in = i < m1, fwd = false;
      uint32_t qp = 0, tp = 0;
      uint64_t qk = 0;
      if (in) {
        const uint32_t mq = match_qi[i], qi = mq & 0x7fffffffu;
        fwd = (mq >> 31) != 0;
        if (fwd) match_qi[i] = qi;
        qp = qpos_of[qi]; tp = idx_pos[match_ti[i]]; qk = mm_key[mm_off[r] + qi];
      }
      unsigned long long mf = __ballot(in && fwd), mr = __ballot(in && !fwd);
      unsigned long long below = (lane == 0) ? 0ULL : (~0ULL >> (64 - lane));
      if (in) {
        uint64_t dst = fwd ? fcur + __popcll(mf & below) : rcur + __popcll(mr & below);
        sep_qpos[dst] = qp; sep_tpos[dst] = tp; sep_qkey[dst] = qk;
      }
      fcur += __popcll(mf); rcur += __popcll(mr);
    }
  }
}

// ------------------------------------------------------------------------------------ scans
// exclusive scan of n (<= a few million) counts into n+1 offsets; one workgroup.

}  // namespace

// ======================================================================================
#include "seed_state.h"

static lra_seed_state* seed_state(lra_ctx* ctx) {
  if (!ctx->seed) ctx->seed = new lra_seed_state();
  return ctx->seed;
}

template <typename T>
static bool regrow(T*& p, size_t n) {
  if (p) (void)hipFree(p);
  p = nullptr;
  return hipMalloc((void**)&p, n * sizeof(T) + 64) == hipSuccess;
}

// a loader on a context that borrows its reference data: the borrowed pointers are dropped (they belong to the owner), the context owns what it loads from here on
static void seed_disown(lra_seed_state* s) {
  if (!s->borrowed) return;
  s->genome = nullptr; s->genome_len = 0; s->idx_key = nullptr; s->idx_pos = nullptr; s->n_idx = 0; s->dir = nullptr; s->nbuckets = 0; s->dir_shift = 0;
  s->borrowed = false; s->owner_cell.reset(); s->owner_generation = 0;
}
// LRA_OK, or LRA_ERR_INVALID when the context borrows reference data its owner has replaced since (lra_ctx_share_reference again)
int lra_seed_check_shared(lra_ctx* ctx) {
  const lra_seed_state* s = ctx->seed;
  if (!s || !s->borrowed || !s->owner_cell) return LRA_OK;
  if (s->owner_cell->dead.load() || s->owner_cell->gen.load() != s->owner_generation)
    return lra_set_err(ctx, LRA_ERR_INVALID, "the context this one shares its reference data with has %s: call lra_ctx_share_reference again",
                       s->owner_cell->dead.load() ? "been destroyed" : "reloaded it");
  return LRA_OK;
}

// lra_ctx_release_buffers: the seed stage's batch arrays (grown to the largest batch's minimizers / matches; the match walk's capacity-spaced buffers are the largest: three
// slots per candidate pair) back to the device, the reference (genome, global index, bucket directory) kept.  -> bytes freed are not tracked per array: the caller reads
// the device's free memory.
void lra_seed_release_batch(lra_ctx* ctx) {
  lra_seed_state* s = ctx->seed;
  if (!s) return;
  void** ptrs[] = {(void**)&s->counts32, (void**)&s->counts64, (void**)&s->mm_off, (void**)&s->match_off, (void**)&s->n_forward, (void**)&s->mm_key, (void**)&s->mm_pos,
                   (void**)&s->lb, (void**)&s->ub, (void**)&s->match_qi, (void**)&s->match_ti, (void**)&s->sep_qpos, (void**)&s->sep_tpos, (void**)&s->tmp_qi, (void**)&s->tmp_ti,
                   (void**)&s->cap_cnt, (void**)&s->cap_off, (void**)&s->tk_lb, (void**)&s->tk_lbm1, (void**)&s->tk_ubm1, (void**)&s->sep_qkey, (void**)&s->defer_flag};
  for (void** p : ptrs) if (*p) { (void)hipFree(*p); *p = nullptr; }
  s->cap_reads = 0; s->cap_mm = 0; s->cap_match = 0; s->cap_tmp = 0; s->cap_defer = 0;
  s->last_n_reads = 0; s->last_n_matches = 0;
}

void lra_seed_free(lra_ctx* ctx) {
  lra_seed_state* s = ctx->seed;
  if (!s) return;
  if (s->borrowed) { s->genome = nullptr; s->idx_key = nullptr; s->idx_pos = nullptr; s->dir = nullptr; }
  else s->cell->dead = true;                                               // borrowers hold the cell, not this state
  void* ptrs[] = {s->genome, s->idx_key, s->idx_pos, s->counts32, s->counts64, s->mm_off, s->match_off, s->n_forward,
                  s->mm_key, s->mm_pos, s->lb, s->ub, s->match_qi, s->match_ti, s->sep_qpos, s->sep_tpos, s->tmp_qi, s->tmp_ti, s->cap_cnt, s->cap_off, s->tk_lb, s->tk_lbm1, s->tk_ubm1, s->dir, s->sep_qkey, s->defer_flag};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  delete s;
  ctx->seed = nullptr;
}

extern "C" int lra_ctx_load_genome(lra_ctx* ctx, const char* h_seq, uint64_t len) {
  if (!ctx || (!h_seq && len)) return LRA_ERR_INVALID;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  lra_seed_state* s = seed_state(ctx);
  seed_disown(s); s->cell->gen++; ctx->ahead.valid = false;   // (a seed result adopted ahead of its batch was made from the old data)
  if (!regrow(s->genome, len + 64)) return lra_set_err(ctx, LRA_ERR_NOMEM, "genome alloc");
  s->genome_len = len;
  LRA_HIP_CHECK(ctx, hipMemcpy(s->genome, h_seq, len, hipMemcpyHostToDevice));
  LRA_HIP_CHECK(ctx, hipMemset(s->genome + len, 0, 64));
  return LRA_OK;
}

// adopts device arrays (hipMalloc'ed, n + 1 entries at least) as the context's global index and builds the bucket directory over the key's top bits
int lra_seed_install_index(lra_ctx* ctx, uint64_t* d_key, uint32_t* d_pos, uint64_t n) {
  lra_seed_state* s = seed_state(ctx);
  seed_disown(s); s->cell->gen++; ctx->ahead.valid = false;   // (a seed result adopted ahead of its batch was made from the old data)
  if (s->idx_key) (void)hipFree(s->idx_key);
  if (s->idx_pos) (void)hipFree(s->idx_pos);
  s->idx_key = d_key; s->idx_pos = d_pos; s->n_idx = n;
  if (!d_key || !d_pos) {
    s->idx_key = nullptr; s->idx_pos = nullptr; s->n_idx = 0;
    if (!regrow(s->idx_key, 2) || !regrow(s->idx_pos, 2)) return lra_set_err(ctx, LRA_ERR_NOMEM, "index alloc");
    n = 0;
  }
  // bucket directory: ~2 buckets per entry, on the top bits of the largest masked key
  int dbits = 1;
  while ((1ULL << dbits) < 2 * n && dbits < 27) dbits++;
  uint64_t maxkey = 0;
  if (n) { LRA_HIP_CHECK(ctx, hipMemcpy(&maxkey, s->idx_key + n - 1, 8, hipMemcpyDeviceToHost)); maxkey &= FOR_MASK; }
  int kbits = 1;
  while (kbits < 63 && (maxkey >> kbits)) kbits++;
  s->dir_shift = kbits > dbits ? kbits - dbits : 0;
  s->nbuckets = (uint32_t)((maxkey >> s->dir_shift) + 1);
  if (!regrow(s->dir, (size_t)s->nbuckets + 2)) return lra_set_err(ctx, LRA_ERR_NOMEM, "index directory");
  hipLaunchKernelGGL(dir_build_kernel, dim3((s->nbuckets + 256) / 256), dim3(256), 0, ctx->stream, s->nbuckets, s->dir_shift, s->idx_key, n, s->dir);
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return LRA_OK;
}

extern "C" int lra_ctx_load_global_index(lra_ctx* ctx, const uint64_t* h_key, const uint32_t* h_pos, uint64_t n) {
  if (!ctx || n >= (1ULL << 32)) return LRA_ERR_INVALID;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  uint64_t* dk = nullptr; uint32_t* dp = nullptr;
  if (!regrow(dk, n + 1) || !regrow(dp, n + 1)) { if (dk) (void)hipFree(dk); return lra_set_err(ctx, LRA_ERR_NOMEM, "index alloc"); }
  LRA_HIP_CHECK(ctx, hipMemcpy(dk, h_key, n * 8, hipMemcpyHostToDevice));
  LRA_HIP_CHECK(ctx, hipMemcpy(dp, h_pos, n * 4, hipMemcpyHostToDevice));
  return lra_seed_install_index(ctx, dk, dp, n);
}

int lra_seed_share(lra_ctx* dst, lra_ctx* src) {
  if (dst->seed && !dst->seed->borrowed && (dst->seed->genome || dst->seed->idx_key)) return lra_set_err(dst, LRA_ERR_INVALID, "context already holds reference data");
  lra_seed_state* d = seed_state(dst);
  const lra_seed_state* s = src->seed;
  d->borrowed = true; d->owner_cell = s->borrowed ? s->owner_cell : s->cell; d->owner_generation = s->borrowed ? s->owner_generation : s->cell->gen.load();
  d->genome = s->genome; d->genome_len = s->genome_len; d->idx_key = s->idx_key; d->idx_pos = s->idx_pos; d->n_idx = s->n_idx;
  d->dir = s->dir; d->nbuckets = s->nbuckets; d->dir_shift = s->dir_shift;
  return LRA_OK;
}

// the context's global index (device arrays; the .mms payload as two columns)
extern "C" int lra_ctx_global_index(lra_ctx* ctx, const uint64_t** d_key, const uint32_t** d_pos, uint64_t* n) {
  if (!ctx || !ctx->seed || !n) return LRA_ERR_INVALID;
  if (d_key) *d_key = ctx->seed->idx_key;
  if (d_pos) *d_pos = ctx->seed->idx_pos;
  *n = ctx->seed->n_idx;
  return LRA_OK;
}

// the genome from a device buffer (copied: the context owns its reference data)
extern "C" int lra_ctx_load_genome_device(lra_ctx* ctx, const char* d_seq, uint64_t len) {
  if (!ctx || (!d_seq && len)) return LRA_ERR_INVALID;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  lra_seed_state* s = seed_state(ctx);
  seed_disown(s); s->cell->gen++; ctx->ahead.valid = false;   // (a seed result adopted ahead of its batch was made from the old data)
  if (!regrow(s->genome, len + 64)) return lra_set_err(ctx, LRA_ERR_NOMEM, "genome alloc");
  s->genome_len = len;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(s->genome, d_seq, len, hipMemcpyDeviceToDevice, ctx->stream));
  LRA_HIP_CHECK(ctx, hipMemsetAsync(s->genome + len, 0, 64, ctx->stream));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return LRA_OK;
}

// CreateRC (SeqUtils.h:151-158, RevCompNuc :112-146): dest[l-i-1] = complement(seq[i]); anything that is
// not one of ACGTacgtn becomes 'N'.
__global__ void create_rc_kernel(int n_reads, const unsigned char* __restrict__ seq, const uint64_t* __restrict__ off, unsigned char* __restrict__ dst) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
  for (int r = wave; r < n_reads; r += nw) {
    const uint64_t a = off[r], L = off[r + 1] - a;
    for (uint64_t i = lane; i < L; i += 64) {
      const unsigned char c = seq[a + i];
      unsigned char o = 'N';
      switch (c) {
        case 'A': o = 'T'; break; case 'C': o = 'G'; break; case 'G': o = 'C'; break; case 'T': o = 'A'; break;
        case 'a': o = 't'; break; case 'c': o = 'g'; break; case 'g': o = 'c'; break; case 't': o = 'a'; break;
        case 'n': o = 'n'; break;
        default: break;
      }
      dst[a + L - 1 - i] = o;
    }
  }
}

extern "C" int lra_create_rc_batch(lra_ctx* ctx, int n_reads, const char* d_seq, const uint64_t* d_read_off, char* d_rc) {
  if (!ctx || n_reads < 0) return LRA_ERR_INVALID;
  if (n_reads == 0) return LRA_OK;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  lra_time_begin(ctx, "create_rc");
  hipLaunchKernelGGL(create_rc_kernel, dim3(ctx->num_cu * 8), dim3(256), 0, ctx->stream, n_reads, (const unsigned char*)d_seq, d_read_off, (unsigned char*)d_rc);
  lra_time_end(ctx);
  LRA_HIP_CHECK(ctx, hipGetLastError());
  return LRA_OK;
}

// the minimizer arrays (and a3's per-minimizer arrays) for total_mm tuples
static int grow_mm(lra_ctx* ctx, lra_seed_state* s, uint64_t total_mm) {
  if (total_mm >= (1ULL << 32)) return lra_set_err(ctx, LRA_ERR_INVALID, "batch too large: %llu minimizers", (unsigned long long)total_mm);
  if (total_mm > s->cap_mm) {
    size_t c = total_mm + total_mm / 4 + 1024;
    if (!regrow(s->mm_key, c) || !regrow(s->mm_pos, c) || !regrow(s->lb, c) || !regrow(s->ub, c) || !regrow(s->tk_lb, c) ||
        !regrow(s->tk_lbm1, c) || !regrow(s->tk_ubm1, c))
      { s->cap_mm = 0; return lra_set_err(ctx, LRA_ERR_NOMEM, "minimizer arrays"); }
    s->cap_mm = c;
  }
  return LRA_OK;
}

// a1 for w > 1: the window machine, a wave per read (sketch_wave_kernel), the reads with a non-ACGT byte a lane per read (sketch_kernel).  The wave kernel lists the
// reads it leaves to the serial one; how many there are comes back with the minimizer total, so a batch without such reads (the usual one) launches nothing for them
// and waits no more often than before.  A batch with some counts them, scans again and reads the total a second time.
static int sketch_windows(lra_ctx* ctx, lra_seed_state* s, int n_reads, const unsigned char* seq, const uint64_t* d_read_off, int k, int w, uint64_t& total_mm) {
  hipStream_t st = ctx->stream;
  // ---- a1: count, scan, emit
  const int gridW = n_reads < ctx->num_cu * 32 ? n_reads : ctx->num_cu * 32;
  int* flagN = (int*)s->n_forward;   // reused before a4 writes it
  uint64_t total_bases = 0;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&total_bases, d_read_off + n_reads, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  // (the staging arrays -- 12 bytes per base of the batch -- live in the sparse DP's arena, slot 12: the seed stage comes first in a batch, the arena is dead until the
  // first sparse DP, and what the batch before left there -- IndelRefine's and CalculateStatistics' arrays -- belonged to a result that ends with this call)
  const size_t key_b = ((size_t)total_bases * 8 + 255) & ~(size_t)255, pos_b = ((size_t)total_bases * 4 + 255) & ~(size_t)255;
  char* stg = (char*)lra_ensure(ctx, 12, key_b + pos_b + ((size_t)n_reads + 1) * 4 + 1024);
  if (!stg) return LRA_ERR_NOMEM;
  uint64_t* wkey = (uint64_t*)stg;
  uint32_t* wpos = (uint32_t*)(stg + key_b);
  int* n_flagged = (int*)(stg + key_b + pos_b); int* flagged = n_flagged + 1;   // the reads left to the serial kernel: their number, then the reads
  LRA_HIP_CHECK(ctx, hipMemsetAsync(n_flagged, 0, 4, st));
  lra_time_begin(ctx, "sketch_emit");
  hipLaunchKernelGGL(sketch_wave_kernel<true>, dim3(gridW), dim3(64), 0, st, n_reads, seq, d_read_off, k, w, d_read_off, wkey, wpos, s->counts32, flagN, n_flagged, flagged);
  lra_time_end(ctx);
  int n_flag = 0;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&n_flag, n_flagged, 4, hipMemcpyDeviceToHost, st));
  if (lra_exclusive_scan<uint32_t>(ctx, (long)n_reads, s->counts32, s->mm_off)) return LRA_ERR_HIP;
  total_mm = 0;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&total_mm, s->mm_off + n_reads, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  if (n_flag < 0 || n_flag > n_reads) return lra_set_err(ctx, LRA_ERR_INVALID, "sketch: flagged read count");
  const int nb = (n_flag + 63) / 64;
  if (n_flag) {
    lra_time_begin(ctx, "sketch_serial");
    hipLaunchKernelGGL(sketch_kernel<false>, dim3(nb), dim3(64), 0, st, n_reads, seq, d_read_off, k, w, (const uint64_t*)nullptr,
                       (uint64_t*)nullptr, (uint32_t*)nullptr, s->counts32, (const int*)flagged, n_flag);
    lra_time_end(ctx);
    if (lra_exclusive_scan<uint32_t>(ctx, (long)n_reads, s->counts32, s->mm_off)) return LRA_ERR_HIP;
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&total_mm, s->mm_off + n_reads, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  }
  { int rc = grow_mm(ctx, s, total_mm); if (rc) return rc; }
  lra_time_begin(ctx, "sketch_compact");
  hipLaunchKernelGGL(sketch_compact, dim3(std::min((n_reads + 3) / 4, ctx->num_cu * 32)), dim3(256), 0, st, n_reads, d_read_off, (const uint64_t*)s->mm_off, (const int*)flagN,
                     (const uint64_t*)wkey, (const uint32_t*)wpos, s->mm_key, s->mm_pos);
  lra_time_end(ctx);
  if (n_flag) {
    lra_time_begin(ctx, "sketch_serial");
    hipLaunchKernelGGL(sketch_kernel<true>, dim3(nb), dim3(64), 0, st, n_reads, seq, d_read_off, k, w, s->mm_off, s->mm_key, s->mm_pos,
                       (uint32_t*)nullptr, (const int*)flagged, n_flag);
    lra_time_end(ctx);
  }
  return LRA_OK;
}

// a1 for w = 1 (sketch_all_kernel): count per tile, scan, the reads' offsets, emit.  No staging copy and no compaction: the emit pass writes the final places.
static int sketch_store_all(lra_ctx* ctx, lra_seed_state* s, int n_reads, const unsigned char* seq, const uint64_t* d_read_off, int k, uint64_t& total_mm) {
  hipStream_t st = ctx->stream;
  uint64_t ends[2] = {0, 0};
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&ends[0], d_read_off, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&ends[1], d_read_off + n_reads, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  if (ends[1] < ends[0]) return lra_set_err(ctx, LRA_ERR_INVALID, "read offsets decrease");
  const uint64_t n_tiles = (ends[1] - ends[0] + 63) / 64;
  // (tile counts, masks and their scan -- 20 bytes per 64 bases -- in slot 12, where the window machine stages its lists: dead until the first sparse DP)
  const size_t cnt_b = ((n_tiles + 1) * 4 + 255) & ~(size_t)255, msk_b = ((n_tiles + 1) * 8 + 255) & ~(size_t)255;
  char* tb = (char*)lra_ensure(ctx, 12, cnt_b + msk_b + (n_tiles + 1) * 8 + 1024);
  if (!tb) return LRA_ERR_NOMEM;
  uint32_t* tile_cnt = (uint32_t*)tb;
  uint64_t* tile_mask = (uint64_t*)(tb + cnt_b);
  uint64_t* tile_pre = (uint64_t*)(tb + cnt_b + msk_b);
  // a run of consecutive tiles per wave: waves for twice what the device holds at once (8 per SIMD), and no more (each starts with a search of the read offsets)
  const uint64_t max_waves = (uint64_t)ctx->num_cu * 64;
  const uint64_t tpw = std::max<uint64_t>(1, (n_tiles + max_waves - 1) / max_waves);
  const uint64_t n_waves = (n_tiles + tpw - 1) / tpw;
  const dim3 grid((unsigned)((n_waves + SKA_NT / 64 - 1) / (SKA_NT / 64)));
  if (n_tiles) {
    lra_time_begin(ctx, "sketch_all_count");
    hipLaunchKernelGGL(sketch_all_kernel<false>, grid, dim3(SKA_NT), 0, st, n_tiles, tpw, n_reads, seq, d_read_off, k, tile_cnt, tile_mask, (const uint64_t*)nullptr,
                       (uint64_t*)nullptr, (uint32_t*)nullptr);
    lra_time_end(ctx);
  }
  LRA_HIP_CHECK(ctx, hipMemsetAsync(tile_mask + n_tiles, 0, 8, st));
  if (lra_exclusive_scan<uint32_t>(ctx, (long)n_tiles, tile_cnt, tile_pre)) return LRA_ERR_HIP;
  hipLaunchKernelGGL(sketch_all_offsets, dim3((unsigned)((n_reads + 1 + 255) / 256)), dim3(256), 0, st, n_reads, d_read_off, n_tiles, (const uint64_t*)tile_pre,
                     (const uint64_t*)tile_mask, s->mm_off);
  total_mm = 0;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&total_mm, tile_pre + n_tiles, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  { int rc = grow_mm(ctx, s, total_mm); if (rc) return rc; }
  if (total_mm) {
    lra_time_begin(ctx, "sketch_all_emit");
    hipLaunchKernelGGL(sketch_all_kernel<true>, grid, dim3(SKA_NT), 0, st, n_tiles, tpw, n_reads, seq, d_read_off, k, (uint32_t*)nullptr, (uint64_t*)nullptr,
                       (const uint64_t*)tile_pre, s->mm_key, s->mm_pos);
    lra_time_end(ctx);
  }
  return LRA_OK;
}

extern "C" int lra_seed_batch(lra_ctx* ctx, int n_reads, const char* d_seq, const uint64_t* d_read_off, int k, int w,
                              int max_freq, lra_seed_result* out) {
  if (!ctx || !out || n_reads < 0) return LRA_ERR_INVALID;
  if (k < 1 || k > 32 || w < 1 || w > MAX_W) return lra_set_err(ctx, LRA_ERR_INVALID, "k must be 1..32 and w 1..%d", MAX_W);
  lra_seed_state* s = seed_state(ctx);
  ctx->ahead.valid = false;                                               // (this call overwrites the buffers of a result adopted ahead of its batch, if there is one)
  if (!s->genome || !s->idx_key) return lra_set_err(ctx, LRA_ERR_INVALID, "load genome and global index first");
  { int rcs = lra_seed_check_shared(ctx); if (rcs) return rcs; }
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  memset(out, 0, sizeof(*out));
  out->n_reads = n_reads;
  if (n_reads == 0) return LRA_OK;
  if ((size_t)n_reads > s->cap_reads) {
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    size_t c = (size_t)n_reads + n_reads / 4 + 64;
    if (!regrow(s->counts32, c) || !regrow(s->counts64, c) || !regrow(s->mm_off, c + 1) || !regrow(s->match_off, c + 1) ||
        !regrow(s->n_forward, c) || !regrow(s->cap_cnt, c) || !regrow(s->cap_off, c + 1))
      { s->cap_reads = 0; return lra_set_err(ctx, LRA_ERR_NOMEM, "per-read arrays"); }   // (capacity 0: whatever the failed group holds is re-made by the next call)
    s->cap_reads = c;
  }
  const unsigned char* seq = (const unsigned char*)d_seq;
  const int gridW = n_reads < ctx->num_cu * 32 ? n_reads : ctx->num_cu * 32;
  // ---- a1
  uint64_t total_mm = 0;
  { int rc = w == 1 ? sketch_store_all(ctx, s, n_reads, seq, d_read_off, k, total_mm) : sketch_windows(ctx, s, n_reads, seq, d_read_off, k, w, total_mm); if (rc) return rc; }
  // ---- a2: a read outside the repeats has no k-mer twice among its minimizers, and a list without equal keys has one sorted order only: the radix path takes nearly
  // all reads, the exact (libstdc++-identical) sort the ones with a repeated k-mer.  The temporaries are a3's outputs, not written yet.
  if (total_mm == 0) { int rc = lra_sort_exact_batch(ctx, n_reads, s->mm_off, s->mm_key, s->mm_pos); if (rc) return rc; }
  else { int rc = lra_sort_mostly_unique_batch(ctx, n_reads, s->mm_off, total_mm, s->mm_key, s->mm_pos, s->tk_lb, s->lb, std::min(2 * k, 63)); if (rc) return rc; }
  // ---- a3
  if (total_mm) {
    lra_time_begin(ctx, "index_bounds");
    hipLaunchKernelGGL(bounds_kernel, dim3((unsigned)((total_mm + 255) / 256)), dim3(256), 0, st, total_mm, s->mm_key, s->idx_key, s->n_idx,
                       s->dir, s->nbuckets, s->dir_shift, s->lb, s->ub, s->tk_lb, s->tk_lbm1, s->tk_ubm1);
    lra_time_end(ctx);
  }
  hipLaunchKernelGGL(match_capacity_kernel, dim3(gridW), dim3(64), 0, st, n_reads, s->mm_off, s->lb, s->ub, s->cap_cnt);
  if (lra_exclusive_scan<uint64_t>(ctx, (long)n_reads, s->cap_cnt, s->cap_off)) return LRA_ERR_HIP;
  uint64_t total_cap = 0;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&total_cap, s->cap_off + n_reads, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  if (total_cap > s->cap_tmp) {
    size_t c = total_cap + total_cap / 4 + 1024;
    if (!regrow(s->tmp_qi, c) || !regrow(s->tmp_ti, c)) { s->cap_tmp = 0; return lra_set_err(ctx, LRA_ERR_NOMEM, "match walk buffers (%llu)", (unsigned long long)total_cap); }
    s->cap_tmp = c;
  }
  // reads per wave of the walk (a lane per read): 32 for a full batch (1024 waves; more waves cost more rounds than the divergence of 32 walks costs), fewer for a small one --
  // a batch of 256 contigs as 256 one-lane waves walks 9 % faster than as 8 waves of 32 diverging lanes (-CONTIG: 3787 -> 3461 ms per batch)
  const int FLAT_LANES = std::max(1, std::min(32, n_reads / 1024));
  lra_time_begin(ctx, "compare");
  hipLaunchKernelGGL(compare_kernel, dim3((n_reads + FLAT_LANES - 1) / FLAT_LANES), dim3(64), 0, st, FLAT_LANES, n_reads, s->mm_off, s->mm_key, s->lb, s->ub, s->tk_lb, s->tk_lbm1, s->tk_ubm1, s->idx_key,
                     (long)s->n_idx, (long)max_freq, s->cap_off, s->tmp_qi, s->tmp_ti, s->counts64);
  lra_time_end(ctx);
  if (s->defer_T) {
    if ((size_t)n_reads > s->cap_defer) {
      LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
      if (!regrow(s->defer_flag, (size_t)n_reads + n_reads / 4 + 64)) { s->cap_defer = 0; return lra_set_err(ctx, LRA_ERR_NOMEM, "defer flags"); }
      s->cap_defer = (size_t)n_reads + n_reads / 4 + 64;
    }
    hipLaunchKernelGGL(defer_heavy_kernel, dim3((n_reads + 255) / 256), dim3(256), 0, st, n_reads, s->defer_T, s->counts64, s->defer_flag);
  }
  if (lra_exclusive_scan<uint64_t>(ctx, (long)n_reads, s->counts64, s->match_off)) return LRA_ERR_HIP;
  uint64_t total_m = 0;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&total_m, s->match_off + n_reads, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  if (total_m > total_cap) return lra_set_err(ctx, LRA_ERR_INVALID, "match capacity bound violated (%llu > %llu)", (unsigned long long)total_m, (unsigned long long)total_cap);
  if (total_m > s->cap_match) {
    size_t c = total_m + total_m / 4 + 1024;
    if (!regrow(s->match_qi, c) || !regrow(s->match_ti, c) || !regrow(s->sep_qpos, c) || !regrow(s->sep_tpos, c) || !regrow(s->sep_qkey, c))
      { s->cap_match = 0; return lra_set_err(ctx, LRA_ERR_NOMEM, "match arrays (%llu matches)", (unsigned long long)total_m); }
    s->cap_match = c;
  }
  // ---- a4
  lra_time_begin(ctx, "strand");
  hipLaunchKernelGGL(strand_kernel, dim3(n_reads < 4096 ? n_reads : 4096), dim3(64), 0, st, n_reads, seq, d_read_off, s->genome, k, s->mm_off,
                     s->mm_pos, s->idx_pos, s->match_off, s->cap_off, s->tmp_qi, s->tmp_ti, s->match_qi, s->match_ti, s->sep_qpos, s->sep_tpos, s->n_forward, s->mm_key, s->sep_qkey);
  lra_time_end(ctx);
  LRA_HIP_CHECK(ctx, hipGetLastError());
  s->last_n_reads = n_reads; s->last_n_matches = total_m;
  out->n_minimizers = total_mm; out->n_matches = total_m;
  out->d_mm_off = s->mm_off; out->d_mm_key = s->mm_key; out->d_mm_pos = s->mm_pos;
  out->d_match_off = s->match_off; out->d_match_qi = s->match_qi; out->d_match_ti = s->match_ti;
  out->d_n_forward = s->n_forward; out->d_sep_qpos = s->sep_qpos; out->d_sep_tpos = s->sep_tpos;
  return LRA_OK;
}

// A match list from the caller in the place of a1-a4's: the clean stage (cluster.hip) reads nothing else of the seed state.  Copies only, no kernel.
extern "C" int lra_seed_set_matches(lra_ctx* ctx, int n_reads, const uint64_t* d_match_off, const uint32_t* d_n_forward, const uint32_t* d_qpos, const uint32_t* d_tpos,
                                    const uint64_t* d_qkey, lra_seed_result* out) {
  if (!ctx || n_reads < 0) return LRA_ERR_INVALID;
  if (n_reads > 0 && (!d_match_off || !d_n_forward)) return lra_set_err(ctx, LRA_ERR_INVALID, "match offsets and forward counts are required");
  lra_seed_state* s = seed_state(ctx);
  ctx->ahead.valid = false;                                               // (this call overwrites the buffers of a result adopted ahead of its batch, if there is one)
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (out) { memset(out, 0, sizeof(*out)); out->n_reads = n_reads; }
  s->last_n_reads = 0; s->last_n_matches = 0;
  if (n_reads == 0) return LRA_OK;
  // the CSR is checked on the host: the clean stage indexes the match arrays with it
  std::vector<uint64_t> off((size_t)n_reads + 1);
  std::vector<uint32_t> nf((size_t)n_reads);
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(off.data(), d_match_off, off.size() * 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(nf.data(), d_n_forward, nf.size() * 4, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  if (off[0] != 0) return lra_set_err(ctx, LRA_ERR_INVALID, "match_off[0] must be 0");
  for (int r = 0; r < n_reads; r++)
    if (off[r + 1] < off[r] || (uint64_t)nf[r] > off[r + 1] - off[r])
      return lra_set_err(ctx, LRA_ERR_INVALID, "read %d: match_off must not decrease and n_forward must not exceed the read's matches", r);
  const uint64_t total_m = off[n_reads];
  if (total_m >= (1ULL << 32)) return lra_set_err(ctx, LRA_ERR_INVALID, "too many matches (%llu)", (unsigned long long)total_m);
  if (total_m && (!d_qpos || !d_tpos || !d_qkey)) return lra_set_err(ctx, LRA_ERR_INVALID, "match arrays are required");
  if ((size_t)n_reads > s->cap_reads) {
    size_t c = (size_t)n_reads + n_reads / 4 + 64;
    if (!regrow(s->counts32, c) || !regrow(s->counts64, c) || !regrow(s->mm_off, c + 1) || !regrow(s->match_off, c + 1) ||
        !regrow(s->n_forward, c) || !regrow(s->cap_cnt, c) || !regrow(s->cap_off, c + 1))
      { s->cap_reads = 0; return lra_set_err(ctx, LRA_ERR_NOMEM, "per-read arrays"); }
    s->cap_reads = c;
  }
  if (total_m > s->cap_match || !s->sep_qpos) {
    size_t c = total_m + total_m / 4 + 1024;
    if (!regrow(s->match_qi, c) || !regrow(s->match_ti, c) || !regrow(s->sep_qpos, c) || !regrow(s->sep_tpos, c) || !regrow(s->sep_qkey, c))
      { s->cap_match = 0; return lra_set_err(ctx, LRA_ERR_NOMEM, "match arrays (%llu matches)", (unsigned long long)total_m); }
    s->cap_match = c;
  }
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(s->match_off, d_match_off, ((size_t)n_reads + 1) * 8, hipMemcpyDeviceToDevice, st));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(s->n_forward, d_n_forward, (size_t)n_reads * 4, hipMemcpyDeviceToDevice, st));
  LRA_HIP_CHECK(ctx, hipMemsetAsync(s->mm_off, 0, ((size_t)n_reads + 1) * 8, st));   // no minimizers stand behind these matches
  if (total_m) {
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(s->sep_qpos, d_qpos, total_m * 4, hipMemcpyDeviceToDevice, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(s->sep_tpos, d_tpos, total_m * 4, hipMemcpyDeviceToDevice, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(s->sep_qkey, d_qkey, total_m * 8, hipMemcpyDeviceToDevice, st));
    LRA_HIP_CHECK(ctx, hipMemsetAsync(s->match_qi, 0, total_m * 4, st));
    LRA_HIP_CHECK(ctx, hipMemsetAsync(s->match_ti, 0, total_m * 4, st));
  }
  s->last_n_reads = n_reads; s->last_n_matches = total_m;
  if (out) {
    out->n_matches = total_m;
    out->d_mm_off = s->mm_off; out->d_mm_key = s->mm_key; out->d_mm_pos = s->mm_pos;
    out->d_match_off = s->match_off; out->d_match_qi = s->match_qi; out->d_match_ti = s->match_ti;
    out->d_n_forward = s->n_forward; out->d_sep_qpos = s->sep_qpos; out->d_sep_tpos = s->sep_tpos;
  }
  return LRA_OK;
}

extern "C" int lra_seed_prefetch(lra_ctx* side, int n_reads, const char* d_seq, const uint64_t* d_read_off, int k, int w, int max_freq) {
  if (!side) return LRA_ERR_INVALID;
  side->ahead.valid = false;
  lra_seed_result res;
  int rc = lra_seed_batch(side, n_reads, d_seq, d_read_off, k, w, max_freq, &res);
  if (rc) return rc;
  LRA_HIP_CHECK(side, hipStreamSynchronize(side->stream));               // (the strand pass is queued, not waited for, by lra_seed_batch)
  side->ahead.n_reads = n_reads; side->ahead.d_seq = d_seq; side->ahead.d_read_off = d_read_off; side->ahead.k = k; side->ahead.w = w; side->ahead.max_freq = max_freq;
  side->ahead.res = res; side->ahead.valid = true;
  return LRA_OK;
}

// The two contexts exchange the seed stage's batch buffers (the result's pointers go with them); the reference data, its ownership and the directory stay.
extern "C" int lra_ctx_adopt_seed(lra_ctx* ctx, lra_ctx* side) {
  if (!ctx || !side || ctx == side) return LRA_ERR_INVALID;
  if (ctx->device != side->device) return lra_set_err(ctx, LRA_ERR_INVALID, "the side context is on another device");
  if (!side->ahead.valid) return lra_set_err(ctx, LRA_ERR_INVALID, "the side context holds no prefetched seed result");
  lra_seed_state* a = seed_state(ctx); lra_seed_state* b = seed_state(side);
  { int rcs = lra_seed_check_shared(side); if (rcs) { side->ahead.valid = false; return lra_set_err(ctx, LRA_ERR_INVALID, "the side context's reference data is stale: share it again"); } }
  if (a->genome != b->genome || a->idx_key != b->idx_key || a->idx_pos != b->idx_pos || a->n_idx != b->n_idx)
    return lra_set_err(ctx, LRA_ERR_INVALID, "the side context does not hold this context's reference data (lra_ctx_share_reference)");
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));                 // nothing of the mapping context's last batch still reads its seed buffers
#define SW(f) std::swap(a->f, b->f)
  SW(counts32); SW(counts64); SW(mm_off); SW(match_off); SW(n_forward); SW(cap_reads);
  SW(mm_key); SW(mm_pos); SW(lb); SW(ub); SW(cap_mm); SW(tk_lb); SW(tk_lbm1); SW(tk_ubm1);
  SW(match_qi); SW(match_ti); SW(sep_qpos); SW(sep_tpos); SW(sep_qkey); SW(cap_match);
  SW(last_n_reads); SW(last_n_matches); SW(defer_flag); SW(cap_defer);
  SW(tmp_qi); SW(tmp_ti); SW(cap_tmp); SW(cap_cnt); SW(cap_off);
#undef SW
  ctx->ahead = side->ahead;
  side->ahead.valid = false;
  return LRA_OK;
}

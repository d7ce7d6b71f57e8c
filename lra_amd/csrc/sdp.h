// lra_amd/csrc/sdp.h -- what the files of the first sparse dynamic program (SDP#A; the algorithm and its layout are described in sdp.hip) share: the per-read
// data layout, the kernels' argument structs, the state of one call of the driver, and the host-side launch functions through which the driver reaches the
// kernels of the other files.  The kernels themselves stay in an anonymous namespace inside their file:
//   sdp_points.hip      counting, point generation, the gathers, the gap-cost table, the arena layout kernels
//   sdp_build.hip       the decompositions (sdp_build: count and emit pass, a wave or a 1024-thread workgroup per read)
//   sdp_process.hip     ProcessPoint, one wave per read            } what the two share: sdp_process.h
//   sdp_process_wg.hip  ProcessPoint, one workgroup per LARGE read }
//   sdp_trace.hip       value order, TraceBack, DecidePrimaryChains
//   sdp_diag.hip        the analysis hooks (LRA_SDP_DUMP / _RATIOS / _STAT / _DBG / _BUILD_STAT)
//   sdp.hip             the driver (sdp_run) and the two entry points
#pragma once
#include "common.h"
#include <vector>

namespace lra_sdp {

constexpr int LV = 18;                    // levels per decomposition (distinct rows / columns per read <= 131072); 2 * LV lanes own them
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr int MAXALN = 16;
constexpr int PEN_TAB_WG = 4096, PEN_TAB_WAVE = 2048;   // entries of the gap-cost table (k_pen_table) the workgroup / the wave kernel keeps in LDS
constexpr int TRACE_CAP = 2560;          // sdp_trace walks reads of up to this many anchors in LDS (16-bit fpred, chain, value order + a `used` bit: 15680 bytes a wave)

struct PwlTab { long long stops[25]; float slope[25], inter[25]; int c1, c2; };

struct Ent { long long val; int b; float v; };   // one Di / Ei slot: diagonal, Db / Eb, Dv / Ev   (16 bytes)
struct Node {            // one full sub-problem (SubProblem.h:15-37), 48 bytes
  uint32_t dBase;        // entry index of Di[0] within the read's entries; Ei[0] at dBase + nD
  uint32_t nD, nE;
  int32_t last;
  uint32_t sTop, nBlk;   // sizes of S_1 and Block
  uint32_t stkOff, blkOff;   // where they live, in pairs from the read's pair area (stacks, Blocks, then the growth pool)
  uint32_t stkCap, blkCap;   // their current capacities: 2 nD + 4 and 2 (nD + nE) + 8 pairs to begin with, doubled from the pool on demand
  long long eLast;           // Ei[nE - 1]: the boundary diagonal of a candidate that owns the whole tail (nearly every push is (i, nE)), so that a push needs no load
};

// Everything ProcessPoint touches for one read lies in one contiguous block (sections 256-byte aligned): a wave's working set is a
// couple of megabytes in one place instead of six arrays gigabytes apart (TLB reach).
struct ReadArena { uint64_t base; uint32_t entOff, apOff, stkOff, visOff, blkPair, poolPair, poolPairs, edOff, visPl; };   // base: device address; byte offsets; nodes at 0
// visOff: the visit records (sub-problem id, index in Di / Ei), one PLANE of P records per (family pair, level) the read can have: the row family's visPl & 0xff planes, then
// the column family's visPl >> 8 -- record of point p on plane k at vis[k * P + p].  A family of n distinct rows / columns uses the levels 0 .. ceil(log2 n) (vis_planes);
// the layout kernels bound n by the read's points, or take the exact rows / columns where a launch before them has counted them (Chunk::lines).
// edOff: one 64-bit word per entry -- for a D entry d the diagonal Ei[Db[d]] (static), which Maximization compares every candidate at (SubRountine.h:292): stored
// beside the entry, the candidate scan is ONE round of independent loads instead of two dependent ones
// The pair area at stkOff holds the candidate stacks, then (from pair index blkPair) the Block lists, then (from poolPair) a pool of
// poolPairs pairs.  Re-inserted candidates (`last` moving backwards) let a stack / Block outgrow any fixed multiple of its sub-problem, so
// they start at 2 nD + 4 / 2 (nD + nE) + 8 pairs and double out of the pool when full; a read that exhausts its pool is re-run with 8x, 64x.

struct PtArgs {
  uint64_t nc;
  const uint64_t* cluster_off; const uint64_t* c_start; const uint32_t* c_count; const int32_t* c_strand;
  const uint32_t* q; const uint32_t* t; const int32_t* len;
  const uint32_t* clusRead; const uint64_t* clusFragOff; const uint64_t* clusPtOff; const uint64_t* fragOff; const uint64_t* ptOff;
  const float* rate_in; float rate; int single;
  uint32_t* fq; uint32_t* ft; int32_t* flen; uint32_t* fcl; uint32_t* fai; float* fval; uint32_t* fprevNode; uint32_t* fprevInd; uint8_t* fflags;
  uint8_t* used; uint8_t* fstrand;
  const uint32_t* qe; const uint32_t* te; uint32_t* fqe; uint32_t* fte;   // box mode only
  uint64_t* key1; uint32_t* pay1; uint32_t* iq; uint32_t* it; uint8_t* ifl; uint32_t* ifr; uint32_t* ptRead;
};

struct BuildArgs {
  int r0, n;                                 // reads [r0, r0 + n)
  const uint32_t* order;                     // block b works on read r0 + order[b] (largest first: the longest waves start first)
  const uint64_t* ptOff;
  const uint32_t* hq; const uint32_t* ht; const uint8_t* hfl; const uint32_t* h2; const uint64_t* key3; const uint32_t* pay3;
  uint32_t* scratch;                         // 34 words per point + 64 per read
  uint32_t* cntEntries; uint32_t* cntNodes; uint32_t* cntD; uint32_t* cntV; uint32_t* cntRC;   // [n] (count pass out; cntRC: max(distinct rows, distinct columns))
  uint32_t* lines;                           // [2 n] count pass out: the read's distinct rows, distinct columns (Chunk::lines)
  const ReadArena* ra;                       // emit pass: per-read blocks
  uint32_t* status;
  unsigned long long* stat;                  // LRA_SDP_BUILD_STAT: cycles per pass (set-up, A, C, D, E, F, G, family set-up) summed over the launch's reads; null = off
};

struct ProcArgs {
  int r0, n;
  const uint32_t* order;
  const uint64_t* ptOff; const uint64_t* fragOff;
  const uint8_t* hfl; const uint32_t* hfr;
  const int32_t* flen; float* fval; uint32_t* fprevNode; uint32_t* fprevInd; uint8_t* fflags;
  const float* rate_in; float rate;
  const ReadArena* ra; uint32_t* poolUsed;
  uint32_t* status;
  PwlTab pwl;
  const short* penTab; int penN;           // -w(|d| + 1) for d < penN (k_pen_table); penN = 0: no table
  int dbg;
  int wgNoRing;          // sdp_process_wg: keep the anchors' words at L2 whatever the spans (LRA_SDP_WG_RING=0: tests of that mode)
  char* wgScratch; const uint64_t* wgOff;   // sdp_process_wg: per large read, the anchors' (best predecessor, contributions) words and the points' ranks
  unsigned long long* stat;                 // sdp_process<true> (LRA_SDP_STAT): 32 counters summed over the launch's waves
};

struct TraceArgs {
  int r0, n, numAln, single; float alnthres;
  int boxes, globalK; const uint32_t* fqe; const uint32_t* fte; const int32_t* numAnchors; int32_t* chainNum;   // box mode (DecidePrimaryChains :1587)
  const uint64_t* fragOff; const uint64_t* read_off;
  const uint32_t* fq; const uint32_t* ft; const int32_t* flen; const uint32_t* fcl; const uint32_t* fai;
  const float* fval; const uint32_t* fpred; const uint8_t* fflags; const uint32_t* opay;
  uint8_t* used;
  const ReadArena* ra;
  uint32_t* nChains; uint64_t* chainStart; uint32_t* chainLen; uint32_t* chainBox; float* chainValue;
  uint32_t* ccl; uint32_t* can; uint8_t* clink; uint32_t* cq; uint32_t* ct; int32_t* clen; uint8_t* cstrand; const uint8_t* fstrand;
  const uint32_t* status;
};

namespace {
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// Inclusive prefix sum over the wave: four DPP row shifts (a row = 16 lanes; nothing is shifted in across a row's start), then the two row broadcasts (rows 1 and 3 take
// lane 15 of the row before them, rows 2 and 3 lane 31) -- six VALU operations where six __shfl_up are six dependent trips through the LDS crossbar.
__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
  (void)lane;
#define LRA_DPP_ADD(ctrl_, rmask_) v += __builtin_amdgcn_update_dpp(0, v, (ctrl_), (rmask_), 0xf, false)
  LRA_DPP_ADD(0x111, 0xf);   // row_shr:1
  LRA_DPP_ADD(0x112, 0xf);   // row_shr:2
  LRA_DPP_ADD(0x114, 0xf);   // row_shr:4
  LRA_DPP_ADD(0x118, 0xf);   // row_shr:8
  LRA_DPP_ADD(0x142, 0xa);   // row_bcast:15
  LRA_DPP_ADD(0x143, 0xc);   // row_bcast:31
#undef LRA_DPP_ADD
  return v;
}
__device__ __host__ inline uint32_t al256(uint64_t x) { return (uint32_t)((x + 255) & ~(uint64_t)255); }
// Levels of a decomposition over n distinct lines: a node halves its lines (floor / ceil) until one is left, so level k holds at most ceil(n / 2^k) lines per node and
// the leaves are at level ceil(log2 n) at the latest.  Never more than LV: sdp_build gives a read up (LRA_ST_RANGE) at the first level without a plane.
__device__ __host__ inline uint32_t vis_planes(uint64_t n) {
  uint32_t d = 1;
  while (d < (uint32_t)LV && (uint64_t(1) << (d - 1)) < n) d++;
  return d;
}
// The plane of slot (family pair, level) = fam2 * LV + level among a read's planes (ReadArena::visPl), NONE where the read has no such level
__device__ __forceinline__ uint32_t vis_plane(uint32_t visPl, int slot) {
  const uint32_t plR = visPl & 0xffu, plC = visPl >> 8;
  if (slot < LV) return (uint32_t)slot < plR ? (uint32_t)slot : NONE;
  const uint32_t lv = (uint32_t)(slot - LV);
  return lv < plC ? plR + lv : NONE;
}
// A read's block is found through an address kept in a table (ReadArena::base).  A pointer made from an integer is a FLAT pointer to the compiler: every access through
// it is a flat_load / flat_store, which counts on the LDS counter as well as on the vector-memory one -- so every LDS read (the gap-cost table inside w(), the slot state)
// waits for all the stores in flight (a stack / Block push is followed by exactly that).  Saying that the address is in global memory gives global_load / global_store.
__device__ __forceinline__ char* arena_ptr(uint64_t addr) { return (char*)(__attribute__((address_space(1))) char*)addr; }
}  // namespace

// ---- the driver's state (sdp.hip); the analysis hooks read it.  From here on the library's own, not part of its ABI
#pragma GCC visibility push(hidden)
// A device buffer of counters of an analysis run (LRA_SDP_STAT, LRA_SDP_BUILD_STAT): freed on every way out of the scope that owns it
struct StatBuf {
  unsigned long long* d = nullptr;
  StatBuf() = default;
  StatBuf(const StatBuf&) = delete;
  StatBuf& operator=(const StatBuf&) = delete;
  ~StatBuf() { release(); }
  void alloc(size_t words, hipStream_t st) { release(); if (hipMalloc((void**)&d, words * 8) != hipSuccess) d = nullptr; else (void)hipMemsetAsync(d, 0, words * 8, st); }
  void release() { if (d) (void)hipFree(d); d = nullptr; }
};

struct Call {                                  // one call of sdp_run
  lra_ctx* ctx; hipStream_t st; const lra_sdp_opts* opts; lra_chain_result* out;
  int n_reads; size_t n1;                      // n1 = n_reads + 1
  const uint64_t* d_cluster_off; const uint64_t* d_c_start; const uint32_t* d_c_count; const int32_t* d_c_strand; const uint32_t* d_q; const uint32_t* d_t;
  const int32_t* d_len; const uint64_t* d_read_off; const float* d_rate; const uint32_t* d_qe; const uint32_t* d_te; const int32_t* d_num_anchors;
  bool boxes;                                  // box mode (d_qe != null): clusters are the fragments; d_c_start / d_c_count are null, d_q/d_t/d_qe/d_te/d_len(=Val)/d_c_strand are per box
  PwlTab pw; short* d_penTab; int penN;        // InitPWL; -w as a table for small distances (slot 190), penN = 0: none
  lra_sort_opts sort;                          // the exact sorts of the call (point orders, value order): timed as "sdp_sort" / "sdp_inner_sort", short lists launched apart
  std::vector<uint64_t> h_off, h_frag, h_pt;   // cluster / fragment / point offsets of the reads
  uint64_t NC, NF, NP; size_t nslot;           // clusters, fragments, points; n_reads * NumAln
  // slot 7: clusters and reads
  uint32_t* clusFragCnt; uint32_t* clusPtCnt; uint32_t* clusRead; uint64_t* clusFragOff; uint64_t* clusPtOff; uint64_t* fragOff; uint64_t* ptOff;
  uint32_t* status; uint32_t* nChains; uint64_t* chainStart; uint32_t* chainLen; float* chainValue; uint32_t* chainBox; int32_t* chainNum;
  // slot 8: fragments
  uint32_t* fq; uint32_t* ft; int32_t* flen; uint32_t* fcl; uint32_t* fai; float* fval; uint32_t* fprevNode; uint32_t* fprevInd; uint32_t* ccl; uint32_t* can;
  uint8_t* fflags; uint8_t* used; uint8_t* clink; uint8_t* fstrand; uint8_t* cstrand; uint32_t* cq; uint32_t* ct; int32_t* clen; uint64_t* okey; uint32_t* fqe; uint32_t* fte;
  // slot 9: points
  uint64_t* key1; uint64_t* key2; uint64_t* key3; uint32_t* pay1; uint32_t* pay2; uint32_t* pay3; uint32_t* iq; uint32_t* it; uint32_t* ifr; uint32_t* ptRead;
  uint32_t* hq; uint32_t* ht; uint32_t* hfr; uint32_t* spare; uint8_t* ifl; uint8_t* hfl; uint32_t* opay; uint32_t* fragRead;
  uint64_t totalEntries = 0;
};

struct Chunk {                                 // reads [r0, r1) of the call: one round of decompositions, ProcessPoint, trace
  int r0, r1, nr; uint64_t cp;                 // cp: its points
  // slot 10
  uint32_t* scratch; uint32_t* cntE; uint32_t* cntN; uint32_t* cntD; uint32_t* cntV; uint32_t* cntRC; uint32_t* order; uint32_t* order2; uint32_t* poolUsed;
  uint32_t* lines;                             // per read its distinct rows and columns where a launch has counted them (the count pass, k_big_lines), else 0, 0: the visit planes' bound
  uint64_t* bytes; uint64_t* byteOff; ReadArena* ra;
  std::vector<uint32_t> h_orderAll, h_prev;    // the reads largest first; the reads of the attempt before this one
  BuildArgs ba; StatBuf buildStat;             // (ba.stat = buildStat.d)
  bool onePass;                                // no count pass: blocks from the per-point estimate
  uint64_t totE = 0; uint32_t maxRC = 0;       // entries of the chunk's reads; max(rows, columns) over them: which sdp_process_wg variant serves its large reads
  // the attempts
  std::vector<uint32_t> h_status, h_sub;
  uint32_t* subOrder; int nsub;                // the reads of the coming attempt
  std::vector<uint64_t> woff;                  // the large reads' offsets into their per-anchor words: the source of a queued copy, so it lives here and not in the attempt
};

struct Attempt {                               // one build + ProcessPoint over chunk.subOrder[0, nsub)
  int att, shift, slot;
  const std::vector<uint32_t>* ordAtt;         // chunk.h_orderAll or chunk.h_prev
  int nbig; bool forked, early;                // reads that get a workgroup each; some of both kinds; the large reads' build and ProcessPoint go first, on the side stream
  bool dbg;
  char* wsc = nullptr; uint64_t* dwoff = nullptr; uint32_t* d_maxLines = nullptr;   // the large reads' per-anchor words (see sdp_process_wg)
  uint64_t totB = 0; uint32_t bigLines = 0;    // read back from the device: they outlive the wait behind the layout
  ProcArgs pa;
  uint64_t dbgOff0 = 0; char* dbgBase = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;       // LRA_SDP_DBG
};

// ---- sdp_points.hip: one function per launch site, the kernel's arguments behind the stream (and the grid's count where the kernel does not take it)
void launch_cluster_counts(hipStream_t st, uint64_t nc, const uint32_t* c_count, uint32_t* fragCnt, uint32_t* ptCnt, int single);
void launch_read_offsets(hipStream_t st, int n_reads, const uint64_t* cluster_off, const uint64_t* clusFragOff, const uint64_t* clusPtOff, uint64_t* fragOff, uint64_t* ptOff,
                         uint32_t* clusRead, uint32_t* status, uint32_t* nChains);
void launch_points(hipStream_t st, const PtArgs& pa);
void launch_frag_read(hipStream_t st, int n_reads, const uint64_t* fragOff, uint32_t* fragRead);
void launch_gather(hipStream_t st, uint64_t np, const uint32_t* ptRead, const uint64_t* ptOff, const uint32_t* pay1, const uint32_t* iq, const uint32_t* it, const uint8_t* ifl,
                   const uint32_t* ifr, uint32_t* hq, uint32_t* ht, uint8_t* hfl, uint32_t* hfr, uint64_t* key2, uint32_t* pay2, uint64_t* key3, uint32_t* pay3);
void launch_reset_frags(hipStream_t st, int n, int r0, const uint32_t* order, const uint64_t* fragOff, const int32_t* flen, const float* rate_in, float rate, float* fval,
                        uint32_t* fprevNode, uint32_t* fprevInd, uint8_t* fflags, uint32_t* status);
void launch_pen_table(hipStream_t st, const PwlTab& pw, short* tab, int* bad);   // PEN_TAB_WG entries
void launch_arena_estimate(hipStream_t st, int n, int r0, const uint64_t* ptOff, float fE, float fN, uint32_t* cntE, uint32_t* cntN, uint32_t* cntD);
void launch_arena_sizes(hipStream_t st, int n, int r0, const uint64_t* ptOff, const uint32_t* cntE, const uint32_t* cntN, const uint32_t* cntD, const uint32_t* lines, ReadArena* ra,
                        uint64_t* bytes, const uint32_t* order, int shift);
void launch_arena_bases(hipStream_t st, int n, const uint64_t* byteOff, ReadArena* ra, const uint32_t* order, char* arena);
void launch_visit_clear(hipStream_t st, int n, const ReadArena* ra, const uint64_t* byteOff, const uint32_t* order);
void launch_big_lines(hipStream_t st, int n, int r0, const uint32_t* order, const uint64_t* ptOff, const uint32_t* hq, const uint32_t* ht, const uint32_t* h2, uint32_t* maxLines,
                      uint32_t* lines);
// ---- sdp_build.hip: the count (emit = false) or emit pass; a 1024-thread workgroup per read for ba.order[0, n), a wave per read for reads [from, to) of d_order / h_order
void launch_wg_builds(bool emit, hipStream_t st, const BuildArgs& ba, int n);
void launch_small_builds(bool emit, lra_ctx* ctx, const BuildArgs& ba, const uint32_t* d_order, const std::vector<uint32_t>& h_order, const uint64_t* h_pt, int from, int to);
// ---- sdp_process.hip, sdp_process_wg.hip: ProcessPoint for pa.order[0, n); stat: sdp_process<true>; lines: max(rows, columns) over the reads, picks the variant
void launch_process(hipStream_t st, const ProcArgs& pa, int n, bool stat);
void launch_process_wg(hipStream_t st, const ProcArgs& pa, int n, uint32_t lines, bool dbg);
// ---- sdp_trace.hip
void launch_valkeys(hipStream_t st, uint64_t f0, uint64_t n, const float* fval, const uint32_t* fragRead, const uint64_t* fragOff, uint64_t* okey, uint32_t* opay);
void launch_pred(hipStream_t st, uint64_t f0, uint64_t n, int r0, const uint32_t* fragRead, const uint32_t* fprevNode, const uint32_t* fprevInd, const uint32_t* status,
                 const ReadArena* ra, uint32_t* fpred);
void launch_trace(hipStream_t st, const TraceArgs& ta);
// ---- sdp_diag.hip: the analysis hooks, each called where the driver's production steps leave room for it; off unless its environment switch is set
bool diag_dbg();                                                      // LRA_SDP_DBG, read once per process
int diag_stat_level();                                                // LRA_SDP_STAT, read once per process
bool diag_build_stat();                                               // LRA_SDP_BUILD_STAT, read once per process
int diag_dump(const Call& c);                                         // LRA_SDP_DUMP: the inputs of the call's largest jobs + all job sizes (tools/sdp_case_stats.py)
void diag_ratios(const Call& c, const Chunk& k);                      // LRA_SDP_RATIOS: entries / nodes / D entries per point over the chunk's reads
void diag_stat(const Call& c, const Attempt& a, int n, StatBuf& s);   // LRA_SDP_STAT: the counters of sdp_process<true> over its n reads; releases s
void diag_dbg_begin(const Call& c, Attempt& a);                       // LRA_SDP_DBG: ProcessPoint's time and the largest read's per-wave table
void diag_dbg_end(const Call& c, const Chunk& k, Attempt& a);
void diag_build_stat(const Call& c, Chunk& k);                        // LRA_SDP_BUILD_STAT: cycles per pass of the mid-size builds; releases k.buildStat
#pragma GCC visibility pop

}  // namespace lra_sdp

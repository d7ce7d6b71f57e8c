// lra_amd/csrc/sdp_process_wg.hip -- the sparse DP's ProcessPoint with one 1024-thread workgroup per LARGE read (sdp.h lists the files).  gfx950 only.
#include "sdp_process.h"

using namespace lra_sdp;

namespace {

// ---- the same for LARGE reads: one 1024-thread workgroup per read, the (family pair, level) slots spread over its 16 waves.
// A read from a satellite array gives tens of thousands of anchors on a lattice of tied rows / columns / diagonals; with one wave per read the
// owners of a start point's insertions take turns (phase 1b above) and every turn is a chain of dependent memory round trips: 44 k points took
// 1.2 s, the whole launch waiting for that one wave.  Here wave w owns the slots w and w + 16: every sub-problem still sees exactly the deposits
// and queries it sees above, in the same order (a sub-problem belongs to one slot, a slot to one wave).  The waves do NOT meet at the points:
// each runs through all points for its own slots.  What couples them is Value[] only -- a start point's candidates from all slots are reduced
// to (max value, first in visit order), and an end point deposits its anchor's value.  So a start point's wave folds its slots' candidates
// into one 64-bit word per (anchor, start point) with atomicMax (value bits high, ~visit rank low: the maximum IS the reference's choice) and
// counts itself in; an end point's wave waits until all 16 waves are counted in for the start points of that anchor that precede it (always
// earlier in every wave's sequence, so the wave that is furthest behind never waits), then takes the value.  fval / prev are written once at
// the end.  The critical path is the busiest wave's own work instead of (slowest wave + two barriers + a serial reduction) per point.
// What a visit costs is its chain of dependent memory round trips (a 47 k-point read from a satellite array: 19 per query of a top-level sub-problem, ~0.65 us
// each, 12 us per point).  So the slot keeps, in LDS, what the next visit will ask memory for: beside the stack top its Di / Ei[y - 1] / Dv (Dv dropped when a
// deposit lands on that entry), the entry below the top with its Di / Ei[y - 1] (position 0 is always the dummy pair), and the sub-problem's Ei[nE - 1] (a push
// nearly always owns the whole tail).  A pop then costs one load (the new top's Dv) instead of three dependent ones, a candidate that beats the top without
// popping costs none, the candidate scan is one round (Ei[Db] stored beside the entries by sdp_build), and the query's E entry is in flight one point ahead.
struct SlotState {
  Node cn; uint32_t cId; int dirty;                // dirty: cn's changing fields are newer than the descriptor in memory (written back when the slot leaves the sub-problem)
  int2 cTop, cLastB; int cTopOk;                  // stack top, last Block pair (valid when cTopOk)
  int topInfoOk, topDvOk; float topDv, topWe; long long topDi;   // of cTop: Di[x], w(Di[x], Ei[n - 1]); Dv[x] while no deposit has touched it
  int2 sec; int secOk, secDvOk; float secDv, secWe; long long secDi;    // the pair below the top, with the same
};
constexpr int WG_NW = 16;
constexpr int RING_W = 2048, RING_LEAD = 1024, RING_CHECK = 32;   // window mode of sdp_process_wg

// Which slots a wave owns.  The cost of a slot falls with its level (measured on a 47 k-point read: R0-R3 and C0-C2 ~ 350-400 M cycles each, level 8 ~ 100 M,
// level 13+ ~ 0), so wave w takes row-family level w and column-family level 15 - w (plus the two levels beyond 15): the busiest wave carries ~ 460 M cycles
// instead of ~ 760 M with slots w, w + 16, w + 32.
__device__ __forceinline__ int wg_slot(int wave, int k) {
  static_assert(LV == 18 && WG_NW == 16, "slot table written for 18 levels on 16 waves");
  if (k == 0) return wave;                                   // R level wave
  if (k == 1) return LV + (15 - wave);                       // C level 15 - wave
  return wave == 0 ? 16 : wave == 1 ? 17 : wave == 15 ? LV + 16 : wave == 14 ? LV + 17 : 2 * LV;   // R16, R17, C16, C17; else none
}

// SPW: slots per wave -- 3 in general (36 slots on 16 waves); 2 when the launch's reads have at most 2^15 distinct rows and columns (levels 16 and 17 are empty then:
// every array per slot is a third smaller, which is what the register file is short of)
// DBG (LRA_SDP_DBG): cycle counters per slot and section; a separate instantiation, because the counters' registers are what the production kernel is short of
template <int SPW, bool DBG>
__global__ void __launch_bounds__(64 * WG_NW) sdp_process_wg(ProcArgs a) {
  __shared__ float s_slope[25], s_inter[25];
  __shared__ SlotState ss[2 * LV];
  __shared__ short s_pen[PEN_TAB_WG];
  // the window of anchors in progress (see below): per start point of an anchor the waves' best candidate and how many waves are counted in
  __shared__ unsigned long long r_best[2 * RING_W];
  __shared__ uint32_t r_cnt[2 * RING_W];
  __shared__ int s_pos[WG_NW]; __shared__ uint32_t s_span, s_wtot[WG_NW];
  __shared__ uint32_t s_bad;       // (read with BAD(): a volatile read is a FLAT load that waits for every outstanding store of the wave, at every point)
#define BAD() __hip_atomic_load(&s_bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
  const int tid = threadIdx.x, lane = tid & 63, wave = u_i(tid >> 6);
  if (tid < 25) { s_slope[tid] = a.pwl.slope[tid]; s_inter[tid] = a.pwl.inter[tid]; }
  const int penN = min(a.penN, PEN_TAB_WG);
  for (int x = tid; x < penN; x += 64 * WG_NW) s_pen[x] = a.penTab[x];
  if (tid < 2 * LV) {
    SlotState z; memset(&z, 0, sizeof z); z.cn.last = -1; z.cId = NONE;
    ss[tid] = z;
  }
  if (tid == 0) { s_bad = 0; s_span = 0; }
  if (tid < WG_NW) s_pos[tid] = 0;
  for (int x = tid; x < 2 * RING_W; x += 64 * WG_NW) { r_best[x] = 0; r_cnt[x] = 0; }
  __syncthreads();
  const int c1 = a.pwl.c1, c2 = a.pwl.c2;
  const int rr = (int)a.order[blockIdx.x], r = a.r0 + rr;
  if (a.status[r] & LRA_ST_CAPACITY) return;                             // (given up by the emit pass, see sdp_process)
  const uint64_t p0 = a.ptOff[r], f0 = a.fragOff[r];
  const int P = (int)(a.ptOff[r + 1] - p0);
  const float rate = a.rate_in ? a.rate_in[r] : a.rate;
  const ReadArena A = a.ra[rr];
  char* ab = arena_ptr(A.base);
  Node* nodes = (Node*)ab;
  Ent* ent = (Ent*)(ab + A.entOff);
  uint32_t* Ap = (uint32_t*)(ab + A.apOff);
  const long long* Ed = (const long long*)(ab + A.edOff);
  int2* pairs = (int2*)(ab + A.stkOff);
  const uint32_t poolPair = A.poolPair, poolPairs = A.poolPairs;
  uint32_t* poolUsed = a.poolUsed + rr;
  const uint2* visR = (const uint2*)(ab + A.visOff);               // the visit planes (ReadArena): a wave reads the planes of its own slots only
  // ---- per anchor: best[2] (one word per start point: value bits << 32 | ~visit rank; 0 = no candidate), cnt[2] (waves counted in), nS, sPos[2];
  // per point: pm = how many start points of its anchor precede it (2 bits), and in window mode the anchor's ordinal and whether it has one start point only
  //
  // WINDOW MODE.  An anchor's words are in use from its first start point to its last end point, `span` points at most; a wave cannot pass an end point before all
  // waves are through its anchor's start points, so the waves stay within a few spans of each other wherever it matters and only the anchors of a window of points are
  // in progress at any time.  Their words then live in LDS -- entry (ordinal of the anchor among first start points) mod RING_W -- instead of at L2: counting in and
  // asking whether all are counted in cost an LDS access instead of dependent L2 round trips.  Entries are never cleared: the count of an entry grows by 16 per
  // generation (ordinal / RING_W; an anchor with one start point counts for both), and a candidate carries its generation above its value, so the maximum is the
  // current generation's.  Anchor o + RING_W must not be counted in while anchor o is in progress: a wave that runs ahead where it has no end points of its own
  // to stop at is held RING_LEAD points in front of the slowest (checked every RING_CHECK points); first start points are distinct points, so o + RING_W starts
  // RING_W points after o at least, and RING_W >= RING_LEAD + RING_CHECK + span + 1 keeps them apart.  Reads with longer spans use the words at L2.
  const int F = (int)(a.fragOff[r + 1] - f0);
  char* wsb = a.wgScratch + a.wgOff[blockIdx.x];
  unsigned long long* best = (unsigned long long*)wsb;
  uint32_t* cnt = (uint32_t*)(wsb + 16 * (size_t)F);
  uint32_t* nS = cnt + 2 * (size_t)F;
  uint32_t* sPos = nS + F;
  uint32_t* pm = sPos + 2 * (size_t)F;
  for (int f = tid; f < F; f += 64 * WG_NW) { best[2 * f] = 0; best[2 * f + 1] = 0; cnt[2 * f] = 0; cnt[2 * f + 1] = 0; nS[f] = 0; sPos[2 * f] = 0; sPos[2 * f + 1] = 0; }
  __syncthreads();
  for (int pi = tid; pi < P; pi += 64 * WG_NW) {
    const uint32_t lf = a.hfr[p0 + pi];
    if (a.hfl[p0 + pi] & 1) { const uint32_t k = atomicAdd(&nS[lf], 1u); if (k < 2) sPos[2 * lf + k] = (uint32_t)pi; else atomicOr(&s_bad, (uint32_t)LRA_ST_RANGE); }
    else atomicMax(&cnt[2 * lf], (uint32_t)pi);                            // (for now: the anchor's last end point)
  }
  __syncthreads();
  for (int f = tid; f < F; f += 64 * WG_NW) {
    if (nS[f] == 2 && sPos[2 * f] > sPos[2 * f + 1]) { const uint32_t t = sPos[2 * f]; sPos[2 * f] = sPos[2 * f + 1]; sPos[2 * f + 1] = t; }
    if (nS[f] > 0 && cnt[2 * f] > sPos[2 * f]) atomicMax(&s_span, cnt[2 * f] - sPos[2 * f]);
    cnt[2 * f] = 0;
  }
  __syncthreads();
  const bool ring = a.wgNoRing == 0 && s_span + RING_LEAD + RING_CHECK + 1 <= (uint32_t)RING_W;
  if (ring) {                                                              // ordinals of the anchors, in the order of their first start points -> cnt[2 f]
    const int per = (P + 64 * WG_NW - 1) / (64 * WG_NW), b0 = min(P, tid * per), b1 = min(P, b0 + per);
    uint32_t mine = 0;
    for (int pi = b0; pi < b1; pi++) mine += (a.hfl[p0 + pi] & 1) && sPos[2 * a.hfr[p0 + pi]] == (uint32_t)pi;
    uint32_t inc = mine;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o); if (lane >= o) inc += t; }
    if (lane == 63) s_wtot[wave] = inc;
    __syncthreads();
    uint32_t at = inc - mine;
    for (int w = 0; w < wave; w++) at += s_wtot[w];
    for (int pi = b0; pi < b1; pi++) { const uint32_t lf = a.hfr[p0 + pi]; if ((a.hfl[p0 + pi] & 1) && sPos[2 * lf] == (uint32_t)pi) cnt[2 * lf] = at++; }
    __syncthreads();
  }
  for (int pi = tid; pi < P; pi += 64 * WG_NW) {
    const uint32_t lf = a.hfr[p0 + pi];
    uint32_t k = 0;
    for (uint32_t x = 0; x < min(nS[lf], 2u); x++) k += sPos[2 * lf + x] < (uint32_t)pi;
    pm[pi] = ring ? (cnt[2 * lf] << 3) | (nS[lf] == 1 ? 4u : 0u) | k : k;
  }
  __threadfence();
  __syncthreads();
  // LRA_SDP_DBG: cycles per wave spent in each of its slots and waiting at end points (16 words per wave behind pm[], 8-aligned)
  unsigned long long* dbgT = (unsigned long long*)(((uintptr_t)(pm + P) + 7) & ~(uintptr_t)7);
  unsigned long long tRounds = 0, tEvents = 0, tStore = 0, tEvA = 0, tEvB = 0, tEvC = 0, tSwitch = 0, tDep = 0, tPub = 0;   // event loop: choosing the candidate, up to the comparison with the top, the winner's path
  unsigned long long tSlot[4] = {0, 0, 0, 0}, tSec[4] = {0, 0, 0, 0};   // tSec (queries only): set-up, Maximization, flush + Block search, result + state
  static_assert(SPW == 2 || SPW == (2 * LV + WG_NW - 1) / WG_NW, "slots per wave");
  // The rows of the points: this point's are scalars, the next point's too (so that ITS sub-problem descriptors and its anchor's value can be asked for now), and
  // the rows of the point after next are in flight in vector registers.  Memory returns in order: what was asked for at the top of the previous point is there
  // by the time anything of this point has been waited for, so a point starts without a round trip of its own.
  uint2 vN[SPW]; uint32_t flN = P > 0 ? u_u(a.hfl[p0]) : 0, lfN = P > 0 ? u_u(a.hfr[p0]) : 0, rkN = P > 0 ? u_u(pm[0]) : 0;
  uint32_t visAt[SPW];                                                   // first record of slot k's plane; NONE: no such slot, or a level the read has no plane for
#pragma unroll
  for (int k = 0; k < SPW; k++) {
    const int slot = wg_slot(wave, k);
    const uint32_t pl = slot < 2 * LV ? vis_plane(A.visPl, slot) : NONE;
    visAt[k] = pl != NONE ? pl * (uint32_t)P : NONE;
    vN[k] = (P > 0 && visAt[k] != NONE) ? u_u2(visR[visAt[k]]) : make_uint2(NONE, 0);
  }
  uint2 vV[SPW]; uint32_t lfV = 0, rkV = 0; uint8_t flV = 0;   // (a byte stays a byte until it is used: widening one waits for its load)
  //                    // raw (per-lane copies of) the rows of point pi + 1 at the top of point pi
#pragma unroll
  for (int k = 0; k < SPW; k++) vV[k] = make_uint2(NONE, 0);
  if (P > 1) {
    flV = a.hfl[p0 + 1]; lfV = a.hfr[p0 + 1]; rkV = pm[1];
#pragma unroll
    for (int k = 0; k < SPW; k++) if (visAt[k] != NONE) vV[k] = visR[visAt[k] + 1u];
  }
  uint32_t ndV[SPW], pfId[SPW]; float fvV = 0.f;                          // asked for one point ahead: lane l < 12 holds word l of the descriptor pfId[k]; the anchor's value
#pragma unroll
  for (int k = 0; k < SPW; k++) { ndV[k] = 0; pfId[k] = NONE; }
  if (P > 0) fvV = a.fval[f0 + lfN];
  constexpr int NODE_WORDS = (int)(sizeof(Node) / 4);
  static_assert(sizeof(Node) % 4 == 0 && NODE_WORDS <= 64 && offsetof(SlotState, cn) == 0, "a descriptor is moved a word per lane");
  const unsigned long long tAll0 = DBG ? clock64() : 0;
  for (int pi = 0; pi < P && !BAD(); pi++) {
    const uint32_t fl = flN, lf = lfN, rk = rkN & 3u;
    const uint32_t re = 2 * ((rkN >> 3) & (uint32_t)(RING_W - 1)), gen = (rkN >> 3) / (uint32_t)RING_W + 1, single = (rkN >> 2) & 1u;   // window mode: the anchor's entry
    const float fvC = fvV;
    const unsigned long long tp0 = DBG ? clock64() : 0;
    if (ring && (pi & (RING_CHECK - 1)) == 0 && lane == 0) {             // not further than RING_LEAD points in front of the slowest wave
      __hip_atomic_store(&s_pos[wave], pi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      for (;;) {
        int mn = pi;
        for (int w = 0; w < WG_NW; w++) mn = min(mn, __hip_atomic_load(&s_pos[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        if (pi - mn <= RING_LEAD || BAD()) break;
        __builtin_amdgcn_s_sleep(8);
      }
    }
    uint2 vv[SPW]; Ent e0[SPW];
#pragma unroll
    for (int k = 0; k < SPW; k++) vv[k] = vN[k];
    const int ind = fl & 1;
    // sub-problem descriptors of this point's visits
    bool act[SPW];
#pragma unroll
    for (int k = 0; k < SPW; k++) {
      const int slot = wg_slot(wave, k);
      act[k] = slot < 2 * LV && vv[k].x != NONE;
      if (act[k] && vv[k].x != u_u(ss[slot].cId)) {
        SlotState& Zs = ss[slot];
        if (lane == 0 && Zs.dirty) { Node* op = nodes + Zs.cId; op->last = Zs.cn.last; op->sTop = Zs.cn.sTop; op->nBlk = Zs.cn.nBlk; op->stkOff = Zs.cn.stkOff; op->stkCap = Zs.cn.stkCap; op->blkOff = Zs.cn.blkOff; op->blkCap = Zs.cn.blkCap; Zs.dirty = 0; }
        uint32_t w = ndV[k];
        if (pfId[k] != vv[k].x && lane < NODE_WORDS) w = ((const uint32_t*)(nodes + vv[k].x))[lane];   // (the first point; otherwise asked for at the previous one)
        if (lane < NODE_WORDS) ((uint32_t*)&Zs)[lane] = w;
        if (lane == 0) { Zs.cId = vv[k].x; Zs.cTopOk = 0; Zs.topInfoOk = 0; Zs.topDvOk = 0; Zs.secOk = 0; Zs.secDvOk = 0; }
      }
    }
    wave_sync();
    if (pi + 1 < P) {                                                    // the next point's rows arrive as scalars; the rows of the one after are asked for
      flN = u_u(flV); lfN = u_u(lfV); rkN = u_u(rkV);
#pragma unroll
      for (int k = 0; k < SPW; k++) vN[k] = u_u2(vV[k]);
      if (pi + 2 < P) {
        flV = a.hfl[p0 + pi + 2]; lfV = a.hfr[p0 + pi + 2]; rkV = pm[pi + 2];
#pragma unroll
        for (int k = 0; k < SPW; k++) if (visAt[k] != NONE) vV[k] = visR[visAt[k] + (uint32_t)(pi + 2)];
      }
      // ... and what the next point will start with: the descriptors of the sub-problems its slots move to (never the ones the slots are in now: those are newer
      // here than in memory; one a slot has left was written back above or earlier, ahead of this load), and its anchor's value if it is an end point
#pragma unroll
      for (int k = 0; k < SPW; k++) {
        const int slot = wg_slot(wave, k);
        pfId[k] = NONE;
        if (slot < 2 * LV && vN[k].x != NONE && vN[k].x != u_u(ss[slot].cId)) {
          pfId[k] = vN[k].x;
          if (lane < NODE_WORDS) ndV[k] = ((const uint32_t*)(nodes + vN[k].x))[lane];
        }
      }
      if (!(flN & 1)) fvV = a.fval[f0 + lfN];
    }
    if (DBG) { __builtin_amdgcn_s_waitcnt(0); tSwitch += clock64() - tp0; }
    float depVal = 0.f;
    if (!ind) {                                                          // an end point: its anchor's value, once every wave has been through its start points
      bool any = false;
#pragma unroll
      for (int k = 0; k < SPW; k++) any |= act[k];
      if (!any) continue;
      const unsigned long long tw0 = DBG ? clock64() : 0;
      if (lane == 0) {
        const int need = (int)rk;
        depVal = fvC;
        for (int x = 0; x < need; x++) {
          if (ring) {                                                     // (LDS serves a wave's accesses in order: the count, then the candidate)
            if (DBG) { tStore += 1ull << 32; if (__hip_atomic_load(&r_cnt[re + x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < (uint32_t)WG_NW * gen) tStore++; }   // polls | not ready at the first
            while (__hip_atomic_load(&r_cnt[re + x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < (uint32_t)WG_NW * gen && !BAD()) __builtin_amdgcn_s_sleep(2);
            const unsigned long long key = __hip_atomic_load(&r_best[re + x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const float v = __uint_as_float((uint32_t)(key >> 16));
            if ((uint32_t)(key >> 48) == gen && depVal < v) depVal = v;
          } else {
            if (DBG) { tStore += 1ull << 32; if (__hip_atomic_load(&cnt[2 * lf + x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (uint32_t)WG_NW) tStore++; }
            // (relaxed loads served by L2: an acquire would invalidate the CU's vector cache under all 16 waves at every end point)
            while (__hip_atomic_load(&cnt[2 * lf + x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (uint32_t)WG_NW && !BAD()) __builtin_amdgcn_s_sleep(2);
            const unsigned long long key = __hip_atomic_load(&best[2 * lf + x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const float v = __uint_as_float((uint32_t)(key >> 32));
            if (key && depVal < v) depVal = v;
          }
        }
      }
      if (DBG) tSlot[3] += clock64() - tw0;
    }
    if (ind) {
#pragma unroll
      for (int k = 0; k < SPW; k++) {
        e0[k].b = -1; e0[k].val = 0; e0[k].v = 0;
        if (act[k]) { const Node& nd = ss[wg_slot(wave, k)].cn; e0[k] = ent[u_u(nd.dBase) + u_u(nd.nD) + vv[k].y]; }   // (the slots' loads are independent: one round)
      }
    }
    float wBest = -2.f; int wRank = 0;                                   // this wave's best candidate of the point and its visit rank
    // (one copy of the visit's code for all of the wave's slots: the kernel is several times the instruction cache as it is)
#pragma unroll 1
    for (int k = 0; k < SPW; k++) {
      const int slot = wg_slot(wave, k);
      if (slot >= 2 * LV) continue;
      const uint2 v = k == 0 ? vv[0] : k == 1 ? vv[1] : vv[SPW - 1];
      const Ent e0k = k == 0 ? e0[0] : k == 1 ? e0[1] : e0[SPW - 1];
      if (!(k == 0 ? act[0] : k == 1 ? act[1] : act[SPW - 1])) continue;
      const unsigned long long ts0 = DBG ? clock64() : 0;
      SlotState& Z = ss[slot];
      Node nd;
      { const Node& zn = Z.cn; nd.dBase = u_u(zn.dBase); nd.nD = u_u(zn.nD); nd.nE = u_u(zn.nE); nd.last = u_i(zn.last); nd.sTop = u_u(zn.sTop); nd.nBlk = u_u(zn.nBlk); nd.stkOff = u_u(zn.stkOff);
        nd.blkOff = u_u(zn.blkOff); nd.stkCap = u_u(zn.stkCap); nd.blkCap = u_u(zn.blkCap); nd.eLast = u_ll(zn.eLast); }
      if (ind == 0) {                                                    // PassValueToD1/D2
        if (lane == 0) {
          const float val = depVal;
          const uint32_t e = nd.dBase + v.y;
          if (ent[e].v < val) {
            ent[e].v = val; Ap[e] = lf;
            if (Z.cTopOk && Z.cTop.x == (int)v.y) Z.topDvOk = 0;         // the cached Dv of the stack top (of the pair below it) is stale now
            if (Z.cTopOk && Z.secOk && Z.sec.x == (int)v.y) Z.secDvOk = 0;
          }
        }
        if (DBG) { __builtin_amdgcn_s_waitcnt(0); tDep += clock64() - ts0; }
        continue;
      }
      const int now = u_i(e0k.b);
      const long long ei1 = u_ll(e0k.val);
      const bool need = now != -1;
      const int m = (int)nd.nD, n = (int)nd.nE, i1 = (int)v.y;
      int oTop = (int)nd.sTop, oBlk = (int)nd.nBlk;
      uint32_t oStkOff = nd.stkOff, oBlkOff = nd.blkOff;
      int2* oS = pairs + oStkOff; int2* oB = pairs + oBlkOff;
      int oSCap = (int)nd.stkCap, oBCap = (int)nd.blkCap;
      const Ent* oD = ent + nd.dBase;
      const long long* oEd = Ed + nd.dBase;
      const long long eLast = nd.eLast;
      uint32_t ost = 0;
      const int on = n;
      // EVERY pair on the stack but the dummy at position 0 has the boundary n (SubRountine.h:388-434: the first pair is pushed as (i, n); FindBoundary(prev.second,
      // cur.second, ...) searches [n, n) or, below the dummy, returns Ei.size() -- so every later pair is (i, n) too).  Hence: `Db[i] >= top.second` (:398, :450) never
      // holds, a candidate is compared with the stack at Ei[n - 1] only, FindBoundary never searches, and `i1 < top.second` (:326) always holds.  A pair is its D index x;
      // what the slot keeps of the top and of the pair below it: x, Di[x], w(Di[x], Ei[n - 1]) (static) and Dv[x] (dropped when a deposit lands on x).
      int tx = -1, sx = -1; int2 olastB = make_int2(0, 0);               // tx / sx == -1: the dummy
      bool tInfo = false, tDvOk = false, secOk = false, sInfo = false, sDvOk = false;
      float tDv = 0.f, tWe = 0.f, sDv = 0.f, sWe = 0.f; long long tDi = 0, sDi = 0;
      if (need) {
        if (u_i(Z.cTopOk)) {
          tx = u_i(Z.cTop.x); olastB = u_i2(Z.cLastB); tInfo = u_i(Z.topInfoOk) != 0; tDvOk = u_i(Z.topDvOk) != 0; tDv = u_f(Z.topDv); tDi = u_ll(Z.topDi); tWe = u_f(Z.topWe);
          secOk = u_i(Z.secOk) != 0; sx = u_i(Z.sec.x); sInfo = secOk; sDi = u_ll(Z.secDi); sWe = u_f(Z.secWe); sDvOk = u_i(Z.secDvOk) != 0; sDv = u_f(Z.secDv);
        } else if (oTop > 0) { tx = oTop == 1 ? -1 : u_i(oS[oTop - 1].x); olastB = oBlk > 0 ? u_i2(oB[oBlk - 1]) : make_int2(0, 0); }
      }
      // Di, Dv and w(Di, Ei[n - 1]) of a pair read from memory
#define PAIR_INFO(x_, di_, dv_, we_) do { const Ent d__ = oD[(x_)]; (di_) = u_ll(d__.val); (dv_) = u_f(d__.v); (we_) = W((di_), eLast); } while (0)
      // the pair at stack position oTop - 1 after a pop: the remembered second pair, the dummy at position 0, or memory
#define NEXT_DOWN(x_, infoOk_, di_, we_, dv_, dvOk_) do { if (secOk) { (x_) = sx; (di_) = sDi; (we_) = sWe; (infoOk_) = true; (dv_) = sDv; (dvOk_) = sDvOk; secOk = false; sDvOk = false; } \
                                               else if (oTop - 1 == 0) { (x_) = -1; (infoOk_) = true; (dvOk_) = false; } \
                                               else { (x_) = u_i(oS[oTop - 1].x); (infoOk_) = false; (dvOk_) = false; } } while (0)
      unsigned long long tq = 0;
      if (DBG) { __builtin_amdgcn_s_waitcnt(0); tq = clock64(); tSec[0] += tq - ts0; }
      if (need && now > nd.last) {                                       // Maximization :275-328, the whole wave
        const int olast = nd.last, onow = now;
        bool stop = false;
        for (int i0 = olast + 1; i0 <= onow && !stop && !ost; i0 += 64) {
          const int j = i0 + lane;
          Ent dj; dj.val = 0; dj.b = -1; dj.v = 0;
          long long ej = 0;
          const unsigned long long tl0 = DBG ? clock64() : 0;
          if (j <= onow) { dj = oD[j]; ej = oEd[j]; }                    // Di / Db / Dv and Ei[Db] of 64 candidates: one round
          if (DBG) { __builtin_amdgcn_s_waitcnt(0); tSlot[2] += clock64() - tl0; tRounds++; }
          const int nb = min(64, onow - i0 + 1);
          int t = 0;
          while (t < nb && !ost) {
            const unsigned long long te0 = DBG ? clock64() : 0;
            if (tx != -1) {
              if (!tInfo) { PAIR_INFO(tx, tDi, tDv, tWe); tInfo = true; tDvOk = true; }
              else if (!tDvOk) { tDv = u_f(oD[tx].v); tDvOk = true; }
              bool evt = false;
              if (lane >= t && lane < nb) evt = dj.b == -1 || BEATS(dj.v, dj.val, tDv, tDi, ej);
              const unsigned long long em = __ballot(evt);
              if (!em) break;
              t = __ffsll((long long)em) - 1;
            }
            const int i = i0 + t;
            const int db = rl_i(dj.b, t);
            if (db == -1) { stop = true; break; }
            unsigned long long te1 = 0;
            if (DBG) { tEvents++; te1 = clock64(); tEvA += te1 - te0; }
            const long long di = rl_ll(dj.val, t), edb = rl_ll(ej, t);
            const float dvi = rl_f(dj.v, t);
            bool win = true;                                             // (chosen by the ballot above: it beats the top at Ei[Db[i]] -- unless the top was the dummy)
            if (tx == -1) {                                              // :389-395 (the stack holds the dummy only)
              BPUSH(make_int2(-1, db)); SPUSH(make_int2(i, on));
              sx = -1; secOk = true; sInfo = true; sDvOk = false;
              tx = i; tDv = dvi; tDi = di; tWe = W(di, eLast); tInfo = true; tDvOk = true;
              win = BEATS(dvi, di, tDv, tDi, edb);                        // (a pair against itself, as the reference compares it: never true)
            }
            unsigned long long te2 = 0;
            if (DBG) { te2 = clock64(); tEvB += te2 - te1; }
            if (win) {                                                    // :405
              if (oBlk > 0 && db > olastB.y) BPUSH(make_int2(tx, db));     // (Db[i] < top.second = n always)
              const float wNew = W(di, eLast), sNew = dvi + wNew;         // the candidate at Ei[n - 1]
              int cx = tx; float cDv = tDv, cWe = tWe; long long cDi = tDi; bool cInfo = true, cDvOk = true;
              while (oTop > 0) {                                          // :415-422
                if (cx < 0 || on < 1) { ost |= LRA_ST_OOB_SLOT; break; }
                if (!(sNew > cDv + cWe)) break;
                oTop--;
                if (oTop == 0) { ost |= LRA_ST_OOB_SLOT; break; }
                NEXT_DOWN(cx, cInfo, cDi, cWe, cDv, cDvOk);
                if (cx == -1) break;                                      // the dummy
                if (!cInfo) { PAIR_INFO(cx, cDi, cDv, cWe); cInfo = true; cDvOk = true; }
                else if (!cDvOk) { cDv = u_f(oD[cx].v); cDvOk = true; }
              }
              if (ost) break;
              SPUSH(make_int2(i, on));                                    // FindBoundary: n (see above)
              sx = cx; secOk = cx == -1 || cInfo; sInfo = secOk; sDi = cDi; sWe = cWe; sDv = cDv; sDvOk = cx != -1 && cInfo && cDvOk;
              tx = i; tDv = dvi; tDi = di; tWe = wNew; tInfo = true; tDvOk = true;
            }
            if (DBG) tEvC += clock64() - te2;
            t++;
          }
        }
      }
      // phase 2 (every lane the same values): the flush of Maximization :438-453 (only its `now == m - 1` branch ever pops), FindValueInBlock :322-333 with a
      // wave-cooperative UPPERbound
      float ev = -2.f;
      if (DBG) { __builtin_amdgcn_s_waitcnt(0); const unsigned long long t1 = clock64(); tSec[1] += t1 - tq; tq = t1; }
      if (need && !ost) {
        if (now == m - 1) { while (oTop > 1 && tx != -1 && !ost) { BPUSH(make_int2(tx, on)); oTop--; NEXT_DOWN(tx, tInfo, tDi, tWe, tDv, tDvOk); } }
        int i2 = -1;
        if (!ost && oBlk > 0) {
          if (i1 >= olastB.y) i2 = tx;                                    // (i1 < top.second always)
          else {
            int bx;
            const unsigned lo = coop_upper_block(oB, (unsigned)oBlk, i1, lane, &bx);   // UPPERbound :205-221, Block[lo].first with it
            if ((int)lo < oBlk) i2 = bx;
          }
        }
        if (DBG) { __builtin_amdgcn_s_waitcnt(0); const unsigned long long t1 = clock64(); tSec[2] += t1 - tq; tq = t1; }
        if (ost || i2 < 0 || i2 >= m) ost |= ost ? ost : LRA_ST_OOB_SLOT;
        else {
          float d2v; long long d2d;
          if (i2 == tx && tInfo && tDvOk) { d2v = tDv; d2d = tDi; }
          else { const Ent d2 = oD[i2]; d2v = u_f(d2.v); d2d = u_ll(d2.val); if (i2 == tx && tInfo) { tDv = d2v; tDvOk = true; } }
          ev = u_f(d2v + W(d2d, ei1) + rate * a.flen[f0 + lf]);
          if (lane == 0) {
            Ap[nd.dBase + nd.nD + i1] = (uint32_t)i2;
            Z.dirty = 1;
            Z.cn.last = now; Z.cn.sTop = (uint32_t)oTop; Z.cn.nBlk = (uint32_t)oBlk; Z.cn.stkOff = oStkOff; Z.cn.blkOff = oBlkOff; Z.cn.stkCap = (uint32_t)oSCap; Z.cn.blkCap = (uint32_t)oBCap;
            Z.cTop = make_int2(tx, tx == -1 ? on + 1 : on); Z.cLastB = olastB; Z.cTopOk = 1;
            Z.topInfoOk = tInfo ? 1 : 0; Z.topDvOk = (tInfo && tDvOk) ? 1 : 0; Z.topDv = tDv; Z.topDi = tDi; Z.topWe = tWe;
            Z.secOk = (secOk && sInfo) ? 1 : 0; Z.sec = make_int2(sx, sx == -1 ? on + 1 : on); Z.secDi = sDi; Z.secWe = sWe; Z.secDv = sDv; Z.secDvOk = (secOk && sInfo && sDvOk) ? 1 : 0;
          }
        }
      }
#undef PAIR_INFO
#undef NEXT_DOWN
      if (ost && lane == 0) atomicOr(&s_bad, ost);
      // Value[ii]: visits apply in the order R family deepest level first, then C family; `val < Ev` keeps the first maximum
      const int vr = (slot / LV) * LV + (LV - 1 - slot % LV);
      if (ev > 0.f && (ev > wBest || (ev == wBest && vr < wRank))) { wBest = ev; wRank = vr; }
      if (DBG) { __builtin_amdgcn_s_waitcnt(0); const unsigned long long t1 = clock64(); if (k == 0) tSlot[0] += t1 - ts0; else if (k == 1) tSlot[1] += t1 - ts0; else tSlot[2] += t1 - ts0; tSec[3] += t1 - tq; }
    }
    wave_sync();
    const unsigned long long tb0 = DBG ? clock64() : 0;
    if (ind && lane == 0) {
      const int x = (int)rk;                                              // which start point of the anchor this is
      if (ring) {
        if (wBest > 0.f) (void)__hip_atomic_fetch_max(&r_best[re + x], ((unsigned long long)gen << 48) | ((unsigned long long)__float_as_uint(wBest) << 16) | (unsigned long long)(0xFFFFu - (uint32_t)wRank),
                                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const uint32_t was = __hip_atomic_fetch_add(&r_cnt[re + x], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (single) (void)__hip_atomic_fetch_add(&r_cnt[re + 1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (was + 1 == (uint32_t)WG_NW * gen) {                            // the last wave in: the anchor's candidate of this start point, for the pass at the end
          const unsigned long long key = __hip_atomic_load(&r_best[re + x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if ((uint32_t)(key >> 48) == gen) best[2 * lf + x] = ((key >> 16) & 0xFFFFFFFFull) << 32 | (unsigned long long)(0xFFFFFFFFu - (0xFFFFu - (uint32_t)(key & 0xFFFFu)));
        }
      } else {
      // the candidate is at L2 before the wave counts itself in: the count's operand depends on the max's return value
      uint32_t one = 1u;
      if (wBest > 0.f) {
        const unsigned long long was = __hip_atomic_fetch_max(&best[2 * lf + x], ((unsigned long long)__float_as_uint(wBest) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)wRank),
                                                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        one += (uint32_t)(was == 0xFFFFFFFFFFFFFFFFull);                   // never true: a key's low word is below 2^32 - 1 only ... (value bits of a finite float are not all ones)
      }
      (void)__hip_atomic_fetch_add(&cnt[2 * lf + x], one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    if (DBG) { __builtin_amdgcn_s_waitcnt(0); tPub += clock64() - tb0; }
  }
  if (DBG && lane == 0) {
    unsigned long long* o = dbgT + 16 * wave;
    o[0] = clock64() - tAll0; o[1] = tSlot[3]; o[2] = tSwitch; o[3] = tDep; o[4] = tPub; o[5] = tSec[0]; o[6] = tSec[1]; o[7] = tSec[2]; o[8] = tSec[3];
    o[9] = tEvA; o[10] = tEvB; o[11] = tEvC; o[12] = (tRounds << 32) | tEvents; o[13] = tStore; o[14] = tSlot[0] + tSlot[1] + tSlot[2]; o[15] = 0;
  }
  __syncthreads();
  // Value[], prev: per anchor the start points in order, `val < Ev` (strict) at each
  if (!s_bad) {
    for (int f = tid; f < F; f += 64 * WG_NW) {
      float val = a.fval[f0 + f];
      int win = -1; unsigned long long wkey = 0;
      for (uint32_t x = 0; x < min(nS[f], 2u); x++) {
        const unsigned long long key = best[2 * f + x];
        const float v = __uint_as_float((uint32_t)(key >> 32));
        if (key && val < v) { val = v; win = (int)x; wkey = key; }
      }
      if (win >= 0) {
        const int vr = (int)(0xFFFFFFFFu - (uint32_t)wkey);
        const int slot = (vr / LV) * LV + (LV - 1 - vr % LV);
        const uint32_t pi = sPos[2 * f + win];
        const uint2 v = visR[(uint64_t)vis_plane(A.visPl, slot) * (uint32_t)P + pi];   // (the winner visited on that level: the plane exists)
        a.fval[f0 + f] = val; a.fprevNode[f0 + f] = v.x; a.fprevInd[f0 + f] = v.y;
        a.fflags[f0 + f] = (uint8_t)((slot < LV ? 1 : 0) | (((a.hfl[p0 + pi] >> 1) & 1) ? 2 : 0));
      }
    }
  }
  if (tid == 0 && s_bad) atomicOr(&a.status[r], (uint32_t)s_bad);
#undef BAD
}

}  // namespace

namespace lra_sdp {

// (levels used = ceil(log2(lines)) + 1: up to 2^15 distinct rows and columns stay within levels 0..15)
void launch_process_wg(hipStream_t st, const ProcArgs& pa, int n, uint32_t lines, bool dbg) {
  if (lines <= 32768) { if (dbg) hipLaunchKernelGGL((sdp_process_wg<2, true>), dim3(n), dim3(64 * WG_NW), 0, st, pa); else hipLaunchKernelGGL((sdp_process_wg<2, false>), dim3(n), dim3(64 * WG_NW), 0, st, pa); }
  else { if (dbg) hipLaunchKernelGGL((sdp_process_wg<3, true>), dim3(n), dim3(64 * WG_NW), 0, st, pa); else hipLaunchKernelGGL((sdp_process_wg<3, false>), dim3(n), dim3(64 * WG_NW), 0, st, pa); }
}

}  // namespace lra_sdp

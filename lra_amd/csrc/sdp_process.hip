// lra_amd/csrc/sdp_process.hip -- the sparse DP's ProcessPoint with one wave per read (sdp.h lists the files; the design is described in sdp.hip).  gfx950 only.
#include "sdp_process.h"

using namespace lra_sdp;

namespace {

// One wave per read.  The points are walked in H1 order (ProcessPoint :1015-1171); lane (family pair, level) < 32 owns the
// sub-problem the point touches on that level.  End points (PassValueToD*) are one independent update per lane.  For a start
// point the lanes whose sub-problem has a usable Eb take turns as owner of a wave-cooperative Maximization (:270-345): the
// owner's state is broadcast, all lanes run the (sequential) candidate-list loop in lock step (every lane issues the same stack /
// Block stores, so each sees its own) with the next 64 Di / Dv / Db and
// Ei[Db] prefetched one per lane, and the two binary searches (FindBoundary, FindValueInBlock's UPPERbound) probe six levels
// per memory round.  Value[ii] is then the (max value, first in visit order) reduction the ordered `val < Ev` updates compute.
template <bool STAT>
__global__ void __launch_bounds__(64, 4) sdp_process(ProcArgs a) {
  // STAT (LRA_SDP_STAT): cycles per section of a point's visit and the lengths of its loops, summed over the launch -- an instantiation of its own (the counters' registers)
  __shared__ unsigned long long sT[STAT ? 10 : 1], sC[STAT ? 20 : 1];     // (in LDS: the production kernel's registers are what the counters would take)
  unsigned long long tPrev = 0;
  if (STAT) { if (threadIdx.x < 10) sT[threadIdx.x] = 0; if (threadIdx.x < 20) sC[threadIdx.x] = 0; tPrev = __builtin_amdgcn_s_memtime(); }
#define TICK(k_) do { if (STAT) { if (a.dbg == 2) __builtin_amdgcn_s_waitcnt(0); const unsigned long long t__ = __builtin_amdgcn_s_memtime(); if (threadIdx.x == 0) sT[k_] += t__ - tPrev; tPrev = t__; } } while (0)
#define CNT(k_, x_) do { const unsigned long long x__ = (unsigned long long)(x_); if (threadIdx.x == 0) sC[k_] += x__; } while (0)
#define WMAX(x_) ([&]() { int m__ = (x_); for (int o__ = 32; o__ > 0; o__ >>= 1) m__ = max(m__, __shfl_xor(m__, o__)); return m__; }())
  __shared__ float s_slope[25], s_inter[25];
  __shared__ short s_pen[PEN_TAB_WAVE];
  const int lane = threadIdx.x;
  if (lane < 25) { s_slope[lane] = a.pwl.slope[lane]; s_inter[lane] = a.pwl.inter[lane]; }
  const int penN = min(a.penN, PEN_TAB_WAVE);
  for (int x = lane; x < penN; x += 64) s_pen[x] = a.penTab[x];
  __syncthreads();
  const int c1 = a.pwl.c1, c2 = a.pwl.c2;
  const int rr = (int)a.order[blockIdx.x], r = a.r0 + rr;
  if (a.status[r] & LRA_ST_CAPACITY) return;                             // the emit pass gave the read up (it outgrew its estimated blocks): it is built again
  const uint64_t p0 = a.ptOff[r], f0 = a.fragOff[r];
  const int P = (int)(a.ptOff[r + 1] - p0);
  const float rate = a.rate_in ? a.rate_in[r] : a.rate;
  const ReadArena A = a.ra[rr];
  char* ab = arena_ptr(A.base);
  Node* nodes = (Node*)ab;
  Ent* ent = (Ent*)(ab + A.entOff);
  uint32_t* Ap = (uint32_t*)(ab + A.apOff);
  const long long* Ed = (const long long*)(ab + A.edOff);
  int2* pairs = (int2*)(ab + A.stkOff);                                  // stacks, Blocks and the growth pool of this read
  const uint32_t poolPair = A.poolPair, poolPairs = A.poolPairs;
  uint32_t* poolUsed = a.poolUsed + rr;
  const uint2* visR = (const uint2*)(ab + A.visOff);
  const int fam2 = lane < LV ? 0 : 1, level = lane < LV ? lane : lane - LV;   // lanes >= 2 * LV have no visits
  // The lane's visit plane (ReadArena: vis[plane * P + point]): it streams along its own plane, eight records a 64-byte line.  visAt: the plane's first record, NONE for a
  // lane whose level the read has no plane for -- it loads nothing and holds NONE.
  const uint32_t visPlane = vis_plane(A.visPl, lane);
  const uint32_t visAt = visPlane != NONE ? visPlane * (uint32_t)P : NONE;
  uint32_t bad = 0;
  // per-lane cache of the sub-problem this lane touched last (descriptor, stack top, last Block pair): consecutive points mostly
  // stay in the same sub-problem on the upper levels
  Node cn; cn.dBase = 0; cn.nD = 0; cn.nE = 0; cn.last = -1; cn.sTop = 0; cn.nBlk = 0; cn.stkOff = 0; cn.blkOff = 0; cn.stkCap = 0; cn.blkCap = 0;
  uint32_t cId = NONE;
  int2 cTop = make_int2(0, 0), cLastB = make_int2(0, 0);
  bool cTopOk = false, cDirty = false;
  // The next point's flags and anchor are the same for every lane, and the compiler moves a wave-uniform value to a scalar register where it is MADE: a v_readfirstlane behind
  // the load, i.e. a wait for the load -- one whole memory round trip at the top of every point (a tenth of a point pair's time), with the visit row's load queued behind
  // it.  Read at an index the compiler cannot see through (a zero in a vector register), the two values stay in vector registers while they are in flight and become
  // scalars where they are used, one point later.
  int vz; asm volatile("v_mov_b32_e32 %0, 0" : "=v"(vz));
  uint32_t flN = P > 0 ? a.hfl[p0 + vz] : 0;
  uint32_t lfN = P > 0 ? a.hfr[p0 + vz] : 0;
  // The visit rows run two points ahead, so that at the top of a point the NEXT point's sub-problems are known and their descriptors can be asked for: straight into LDS
  // (global_load_lds_dwordx4: a lane's 16 bytes land at the base + 16 * lane, no vector register is held while the load is in flight -- the registers are what this
  // kernel is short of), three loads for the 48 bytes, two buffers taken in turn.  A lane that moves to another sub-problem finds the descriptor there instead of
  // starting a round trip (every end point's deepest lanes do); never the one the lane is in (newer in its registers than in memory), and one it has left was written back
  // above, ahead of the load.
  static_assert(sizeof(Node) == 48, "a descriptor is fetched as three 16-byte pieces");
  __shared__ uint4 s_node[2][3][2 * LV];
  uint2 vN = make_uint2(NONE, 0), vNN = make_uint2(NONE, 0);
  if (P > 0 && visAt != NONE) vN = visR[visAt];
  if (P > 1 && visAt != NONE) vNN = visR[visAt + 1u];
  // (the lane is in no sub-problem yet: the first point's descriptors, asked for here)
#define NODE_FETCH(id_, buf_) do { const char* src__ = (const char*)(nodes + (id_)); _Pragma("unroll") for (int w__ = 0; w__ < 3; w__++) \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src__ + 16 * w__), (__attribute__((address_space(3))) void*)&s_node[(buf_)][w__][0], 16, 0, 0); } while (0)
  if (vN.x != NONE) NODE_FETCH(vN.x, 0);
  for (int pi = 0; pi < P && !bad; pi++) {
    const uint8_t fl = (uint8_t)u_u(flN);
    const uint32_t lf = u_u(lfN);
    const uint2 v = vN;
    vN = vNN;
    // (whenever a lane moves, the descriptor it moves to was asked for at the point before -- or ahead of the loop --: the only source.  With a second one, a load from
    // memory where the buffer does not hold it, the compiler either folds the two into FLAT loads through a generic pointer or waits for ALL vector memory where the two
    // paths meet.  And the move comes FIRST in the point, the buffer read ahead of the write-back: the compiler waits for all vector memory before it reads what a
    // load wrote to LDS, which costs nothing here -- the point before ended with everything waited for -- and a round trip behind anything asked for earlier in the point)
    bool swd = false;
    if (v.x != NONE && v.x != cId) {
      swd = true;
      const uint4 w0 = s_node[pi & 1][0][lane], w1 = s_node[pi & 1][1][lane], w2 = s_node[pi & 1][2][lane];
      // (the descriptor's changing fields live in this lane's copy while the lane stays in the sub-problem; memory gets them when it leaves: a store per query
      // would be waited for by the next point's loads -- vector memory completes in order)
      if (cDirty) { Node* op = nodes + cId; op->last = cn.last; op->sTop = cn.sTop; op->nBlk = cn.nBlk; op->stkOff = cn.stkOff; op->stkCap = cn.stkCap; op->blkOff = cn.blkOff; op->blkCap = cn.blkCap; cDirty = false; }
      cn.dBase = w0.x; cn.nD = w0.y; cn.nE = w0.z; cn.last = (int32_t)w0.w; cn.sTop = w1.x; cn.nBlk = w1.y; cn.stkOff = w1.z; cn.blkOff = w1.w; cn.stkCap = w2.x; cn.blkCap = w2.y;
      cn.eLast = (long long)(((unsigned long long)w2.w << 32) | w2.z);
      cId = v.x; cTopOk = false;
    }
    if (pi + 1 < P) {                                                    // the rows of the point after next, the next point's flags: in flight while this one is processed
      vNN = make_uint2(NONE, 0);
      if (pi + 2 < P && visAt != NONE) vNN = visR[visAt + (uint32_t)(pi + 2)];
      flN = a.hfl[p0 + pi + 1 + vz]; lfN = a.hfr[p0 + pi + 1 + vz];
    }
    if (vN.x != NONE && vN.x != cId) NODE_FETCH(vN.x, (pi + 1) & 1);      // (lanes >= 2 * LV never have a visit: nothing is written beyond a buffer's 36 slots)
    const int ind = fl & 1, inv = (fl >> 1) & 1;
    const float fvP = a.fval[f0 + lf];                                   // the anchor's value so far (asked for now: the point ends with it)
    if (STAT) { const int sw = __popcll(__ballot(swd)); const int nl = __popcll(__ballot(v.x != NONE)); CNT(ind ? 1 : 0, 1); CNT(ind ? 3 : 2, sw > 0); CNT(ind ? 5 : 4, nl); TICK(ind ? 1 : 0); }
    if (ind == 0) {                                                      // PassValueToD1/D2 (SparseDP.h:140-310)
      if (v.x != NONE) {
        const float val = fvP;
        const uint32_t e = cn.dBase + v.y;
        if (ent[e].v < val) { ent[e].v = val; Ap[e] = lf; }
      }
      TICK(2);
    } else {                                                             // start point (:1025-1060)
      // Every pair on a stack but the dummy at position 0 has the boundary n (see sdp_process_wg): a pair is its D index; `Db >= top.second` never holds,
      // candidates meet the stack at Ei[n - 1] only, FindBoundary never searches.
      // phase 0, every lane for its own sub-problem: Eb[i1], stack top, last Block pair
      const Node& nd = cn;                                                 // (a lane without a visit has need == false below: nothing of nd is used)
      int now = -1;
      long long ei1 = 0;
      const int m = (int)nd.nD, n = (int)nd.nE, i1 = (int)v.y;
      int sTop = (int)nd.sTop, nBlk = (int)nd.nBlk;
      uint32_t stkOff = nd.stkOff, blkOff = nd.blkOff;
      // (stack, Block list, Di, Ei[Db] are addressed from their offsets where they are used: four 64-bit pointers per lane are eight registers)
      int sCap = (int)nd.stkCap, bCap = (int)nd.blkCap;
      const long long eLast = nd.eLast;
      int tx = cTop.x; int2 lastB = cLastB;                               // tx == -1: the dummy
      // sx: the D index of the pair BELOW the top (-1: the dummy is below it; SX_UNK: not known) -- what a pop or the flush would have to read the stack for.  A push makes
      // it known (the top it covers); a pop that leaves two pairs or more above the dummy forgets it.
      constexpr int SX_UNK = -2;
      int sx = cTop.y;
      uint32_t st = 0;
      // what the visit asks memory for first, in ONE round: the query's E entry, the stack top and the last Block pair (when the lane has just come to the sub-problem),
      // the first candidate and the top's D entry (used if the query inserts anything)
      Ent pfD; pfD.val = 0; pfD.b = -1; pfD.v = 0;
      long long pfE = 0;
      Ent pfT; pfT.val = 0; pfT.b = 0; pfT.v = 0;
      bool pfTok = false;
      float pfSv = 0.f; long long pfSd = 0; int pfSx = SX_UNK;            // the D entry of the pair below the top (what the first pop compares with)
      if (v.x != NONE) {
        const Ent e = ent[nd.dBase + nd.nD + v.y];
        int2 sT = make_int2(-1, 0), sS = make_int2(-1, 0), bL = make_int2(0, 0);
        if (!cTopOk) { if (sTop > 1) sT = (pairs + stkOff)[sTop - 1]; if (sTop > 2) sS = (pairs + stkOff)[sTop - 2]; if (nBlk > 0) bL = (pairs + blkOff)[nBlk - 1]; }
        if (nd.last + 1 < m) { pfD = (ent + nd.dBase)[nd.last + 1]; pfE = (Ed + nd.dBase)[nd.last + 1]; }
        if (cTopOk && tx >= 0) { pfT = (ent + nd.dBase)[tx]; pfTok = true; }
        if (cTopOk && sx >= 0) { const Ent es = (ent + nd.dBase)[sx]; pfSv = es.v; pfSd = es.val; pfSx = sx; }
        now = e.b; ei1 = e.val;
        if (!cTopOk) { tx = sTop <= 1 ? -1 : sT.x; sx = sTop <= 2 ? -1 : sS.x; lastB = bL; }
      }
      const bool need = now != -1;
      const int pfTx = pfTok ? tx : SX_UNK;                               // the D index pfT was read for
      const int nBlk0 = nBlk; const uint32_t blkOff0 = blkOff;
      TICK(3);
      // phase 1a, every lane for itself: short insertion runs (most queries advance `now` by a few candidates only) -- the same loop
      // as below, literal and lane-local, all lanes at once
      const int LOCAL_MAX = 4;                                             // (6: 635 ms over 12 launches, 4: 617, 2 / 3: 635, 1: 652, 10: 634, 16: 635)
      const bool small = need && now > nd.last && now - nd.last <= LOCAL_MAX;
      int nIt = 0, nPop = 0;
      if (small) {
        bool topD = false; float tDv = 0; long long tDi = 0;
#define SPUSHL(val_) do { const int2 v__ = (val_); if (sTop >= sCap) { if (!grow_pairs(pairs, stkOff, sCap, sTop, poolUsed, poolPair, poolPairs)) st |= LRA_ST_CAPACITY; } \
                          if (sTop < sCap) (pairs + stkOff)[sTop] = v__; sTop++; } while (0)
#define BPUSHL(val_) do { const int2 v__ = (val_); if (nBlk >= bCap) { if (!grow_pairs(pairs, blkOff, bCap, nBlk, poolUsed, poolPair, poolPairs)) st |= LRA_ST_CAPACITY; } \
                          if (nBlk < bCap) (pairs + blkOff)[nBlk] = v__; nBlk++; lastB = v__; } while (0)
        for (int i = nd.last + 1; i <= now && !st; ++i) {
          if (STAT) nIt++;
          Ent di_ = pfD; long long edb = pfE;
          if (i != nd.last + 1) { di_ = (ent + nd.dBase)[i]; edb = (Ed + nd.dBase)[i]; }
          const int db = di_.b;
          if (db == -1) break;
          const long long di = di_.val; const float dvi = di_.v;
          if (tx == -1) { BPUSHL(make_int2(-1, db)); SPUSHL(make_int2(i, n)); tx = i; sx = -1; tDv = dvi; tDi = di; topD = true; }
          if (!topD) { Ent e = pfT; if (!pfTok) e = (ent + nd.dBase)[tx]; tDv = e.v; tDi = e.val; topD = true; }
          if (BEATS(dvi, di, tDv, tDi, edb)) {
            if (nBlk > 0 && db > lastB.y) BPUSHL(make_int2(tx, db));
            const float sNew = dvi + W(di, eLast);
            int cx = tx; float cDv = tDv; long long cDi = tDi;
            while (sTop > 0) {
              if (cx < 0 || n < 1) { st |= LRA_ST_OOB_SLOT; break; }
              if (!(sNew > cDv + W(cDi, eLast))) break;
              sTop--;
              if (STAT) nPop++;
              if (sTop == 0) { st |= LRA_ST_OOB_SLOT; break; }
              cx = sTop - 1 == 0 ? -1 : sx != SX_UNK ? sx : (pairs + stkOff)[sTop - 1].x;
              sx = sTop - 1 <= 1 ? -1 : SX_UNK;
              if (cx == -1) break;
              if (cx == pfSx) { cDv = pfSv; cDi = pfSd; }
              else { const Ent ce = (ent + nd.dBase)[cx]; cDv = ce.v; cDi = ce.val; }
            }
            if (st) break;
            SPUSHL(make_int2(i, n)); sx = cx; tx = i; tDv = dvi; tDi = di; topD = true;
          }
        }
#undef SPUSHL
#undef BPUSHL
      }
      if (STAT) { const int mi = WMAX(nIt), mp = WMAX(nPop); CNT(6, mi); CNT(7, mp); CNT(8, mi > 0); TICK(4); }
      // phase 1b, one owner at a time, the whole wave: long insertion runs  for (i = last + 1; i <= now; ++i)  of Maximization :275-328
      unsigned long long todo = __ballot(need && now > nd.last && !small);
      if (STAT) CNT(9, __popcll(todo));
      while (todo) {
        const int owner = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const Ent* oD = ent + (uint32_t)rl_i((int)nd.dBase, owner);
        const long long* oEd = Ed + (uint32_t)rl_i((int)nd.dBase, owner);
        const int on = rl_i(n, owner);
        const long long oeLast = rl_ll(eLast, owner);
        const int olast = rl_i(nd.last, owner), onow = rl_i(now, owner);
        int oTop = rl_i(sTop, owner), oBlk = rl_i(nBlk, owner);
        uint32_t oStkOff = (uint32_t)rl_i((int)stkOff, owner), oBlkOff = (uint32_t)rl_i((int)blkOff, owner);
        int2* oS = pairs + oStkOff; int2* oB = pairs + oBlkOff;
        int oSCap = rl_i(sCap, owner), oBCap = rl_i(bCap, owner);
        int otx = rl_i(tx, owner), osx = rl_i(sx, owner); int2 olastB = make_int2(rl_i(lastB.x, owner), rl_i(lastB.y, owner));
        uint32_t ost = 0;
        bool topD = rl_i(pfTok ? 1 : 0, owner) != 0; float tDv = rl_f(pfT.v, owner); long long tDi = rl_ll(pfT.val, owner);   // (the owner's top, asked for above)
        bool stop = false;
        for (int i0 = olast + 1; i0 <= onow && !stop && !ost; i0 += 64) {
          const int j = i0 + lane;
          Ent dj; dj.val = 0; dj.b = -1; dj.v = 0;
          long long ej = 0;
          if (j <= onow) { dj = oD[j]; ej = oEd[j]; }
          const int nb = min(64, onow - i0 + 1);
          int t = 0;
          while (t < nb && !ost) {
            // iterations that neither stop nor beat the top candidate change nothing: every lane tests its own candidate
            // against the current top and the wave jumps to the first one that does something
            if (otx != -1) {
              if (!topD) { const Ent e = oD[otx]; tDv = e.v; tDi = e.val; topD = true; }
              bool evt = false;
              if (lane >= t && lane < nb) evt = dj.b == -1 || BEATS(dj.v, dj.val, tDv, tDi, ej);
              const unsigned long long em = __ballot(evt);
              if (!em) break;
              t = __ffsll((long long)em) - 1;
            }
            const int i = i0 + t;
            const int db = rl_i(dj.b, t);
            if (db == -1) { stop = true; break; }                         // :277
            const long long di = rl_ll(dj.val, t), edb = rl_ll(ej, t);
            const float dvi = rl_f(dj.v, t);
            bool win = true;                                              // (the ballot's test is the reference's, :405, unless the top was the dummy)
            if (otx == -1) { BPUSH(make_int2(-1, db)); SPUSH(make_int2(i, on)); otx = i; osx = -1; tDv = dvi; tDi = di; topD = true; win = BEATS(dvi, di, tDv, tDi, edb); }   // :389-395
            if (win) {
              if (oBlk > 0 && db > olastB.y) BPUSH(make_int2(otx, db));
              const float sNew = dvi + W(di, oeLast);
              int cx = otx; float cDv = tDv; long long cDi = tDi;
              while (oTop > 0) {                                          // :415-422
                if (cx < 0 || on < 1) { ost |= LRA_ST_OOB_SLOT; break; }
                if (!(sNew > cDv + W(cDi, oeLast))) break;
                oTop--;
                if (oTop == 0) { ost |= LRA_ST_OOB_SLOT; break; }
                cx = oTop - 1 == 0 ? -1 : osx != SX_UNK ? osx : oS[oTop - 1].x;
                osx = oTop - 1 <= 1 ? -1 : SX_UNK;
                if (cx == -1) break;
                const Ent ce = oD[cx]; cDv = ce.v; cDi = ce.val;
              }
              if (ost) break;
              SPUSH(make_int2(i, on)); osx = cx; otx = i; tDv = dvi; tDi = di; topD = true;
            }
            t++;
          }
        }
        if (lane == owner) { sTop = oTop; nBlk = oBlk; tx = otx; sx = osx; lastB = olastB; st |= ost; stkOff = oStkOff; blkOff = oBlkOff; sCap = oSCap; bCap = oBCap; }
      }
      TICK(5);
      // phase 2, every lane for its own sub-problem: the flush of Maximization :438-453 (only its `now == m - 1` branch ever pops), FindValueInBlock :322-333, Ev / Ep
      float ev = -1.f;
      bool got = false;
      int nFl = 0, nSr = 0, nLd = 0, nBs = 0, nCh = 0;
      if (need && !st) {
#define BPUSH2(val_) do { const int2 v__ = (val_); if (nBlk >= bCap) { if (!grow_pairs(pairs, blkOff, bCap, nBlk, poolUsed, poolPair, poolPairs)) st |= LRA_ST_CAPACITY; } \
                          if (nBlk < bCap) (pairs + blkOff)[nBlk] = v__; nBlk++; lastB = v__; } while (0)
        if (now == m - 1) {
          while (sTop > 1 && tx != -1 && !st) {
            if (STAT) nFl++;
            BPUSH2(make_int2(tx, n)); sTop--;
            tx = sTop - 1 == 0 ? -1 : sx != SX_UNK ? sx : (pairs + stkOff)[sTop - 1].x;
            sx = sTop - 1 <= 1 ? -1 : SX_UNK;
          }
        }
#undef BPUSH2
        int i2 = -1;
        if (!st && nBlk > 0) {
          if (i1 >= lastB.y) i2 = tx;                                     // (i1 < top.second always)
          else {
            if (STAT) { nBs = nBlk; nCh = (nBlk != nBlk0 || blkOff != blkOff0) ? 1 : 0; }
            int lo = 0, cnt = nBlk, bx = -1;                              // UPPERbound :205-221, two levels per memory round; the search ends at the position of its most
            while (cnt > 0) {                                             // recent false probe (or at the end): Block[lo].first is that probe's pair, no further load
              if (STAT) nSr++;
              const int step = cnt >> 1, it = lo + step;
              const int cntT = cnt - step - 1, itT = it + 1 + (cntT >> 1), itF = lo + (step >> 1);
              const int2 pM = (pairs + blkOff)[it], pT = cntT > 0 ? (pairs + blkOff)[itT] : make_int2(0, 0), pF = step > 0 ? (pairs + blkOff)[itF] : make_int2(0, 0);
              if (i1 >= pM.y) {
                lo = it + 1; cnt = cntT;
                if (cnt > 0) { const int s2 = cnt >> 1; if (i1 >= pT.y) { lo = itT + 1; cnt -= s2 + 1; } else { cnt = s2; bx = pT.x; } }
              } else {
                cnt = step; bx = pM.x;
                if (cnt > 0) { const int s2 = cnt >> 1; if (i1 >= pF.y) { lo = itF + 1; cnt -= s2 + 1; } else { cnt = s2; bx = pF.x; } }
              }
            }
            if (lo < nBlk) i2 = bx;
          }
        }
        if (st || i2 < 0 || i2 >= m) st |= st ? st : LRA_ST_OOB_SLOT;
        else {
          // (the answer is the stack top more often than not, and when nothing was pushed in this visit its D entry came with the visit's first loads)
          Ent d2;
          if (i2 == pfTx) d2 = pfT;
          else if (i2 == pfSx) { d2.v = pfSv; d2.val = pfSd; d2.b = 0; }
          else { d2 = (ent + nd.dBase)[i2]; if (STAT) nLd = 1; }
          ev = d2.v + W(d2.val, ei1) + rate * a.flen[f0 + lf];            // :1040
          got = true;
          Ap[nd.dBase + nd.nD + i1] = (uint32_t)i2;                       // Ep[i1] (Ev[i1] is never read again)
          cDirty = true;
          cn.last = now; cn.sTop = (uint32_t)sTop; cn.nBlk = (uint32_t)nBlk; cn.stkOff = stkOff; cn.blkOff = blkOff; cn.stkCap = (uint32_t)sCap; cn.blkCap = (uint32_t)bCap;
          cTop = make_int2(tx, sx); cLastB = lastB; cTopOk = true;
        }
      }
      if (STAT) { const int mf = WMAX(nFl), ms = WMAX(nSr), ml = WMAX(nLd), mb = WMAX(nBs), mc = WMAX(nCh), m2 = WMAX(nIt >= 2 ? 1 : 0); CNT(10, mf); CNT(11, ms); CNT(12, ml); CNT(13, ms > 0); CNT(14, mc); CNT(15, mb); CNT(16, m2); TICK(6); }
      const uint32_t myI1 = v.y;
      if (__ballot(st != 0)) { for (int o = 32; o > 0; o >>= 1) st |= __shfl_xor(st, o); }   // (a status is rare: no exchange unless a lane has one)
      bad |= st;
      // Value[ii]: visits apply in the order R family deepest level first, then C family; `val < Ev` keeps the first maximum.  The maximum over the lanes by DPP row
      // shifts / broadcasts (six VALU operations; a butterfly of __shfl_xor is twelve dependent trips through the LDS crossbar, a tenth of a point's time), then the
      // first lane in visit order among those that hold it: within a family a higher lane is a deeper level, and the R family's lanes come first
      if (!bad) {
        const float bvM = wave_max_f32(got ? ev : -__builtin_inff());
        const unsigned long long eq = __ballot(got && ev == bvM);
        const unsigned long long eqR = eq & ((1ull << LV) - 1);
        const int win = eq ? 63 - __clzll((long long)(eqR ? eqR : eq)) : -1;
        if (lane == win) {
          if (fvP < ev) {
            a.fval[f0 + lf] = ev; a.fprevNode[f0 + lf] = v.x; a.fprevInd[f0 + lf] = myI1;
            a.fflags[f0 + lf] = (uint8_t)((fam2 == 0 ? 1 : 0) | (inv ? 2 : 0));   // bit0 prev (row family), bit1 inv
          }
        }
      }
      TICK(7);
    }
    wave_sync();
    TICK(ind ? 9 : 8);
  }
  if (STAT && lane == 0 && a.stat) { for (int k = 0; k < 10; k++) atomicAdd(a.stat + k, sT[k]); for (int k = 0; k < 20; k++) atomicAdd(a.stat + 10 + k, sC[k]); }
  if (cDirty && cId != NONE) { Node* op = nodes + cId; op->last = cn.last; op->sTop = cn.sTop; op->nBlk = cn.nBlk; op->stkOff = cn.stkOff; op->stkCap = cn.stkCap; op->blkOff = cn.blkOff; op->blkCap = cn.blkCap; }
  if (lane == 0 && bad) atomicOr(&a.status[r], bad);
#undef NODE_FETCH
#undef TICK
#undef CNT
#undef WMAX
}

}  // namespace

namespace lra_sdp {

void launch_process(hipStream_t st, const ProcArgs& pa, int n, bool stat) {
  if (stat) hipLaunchKernelGGL(sdp_process<true>, dim3(n), dim3(64), 0, st, pa);
  else hipLaunchKernelGGL(sdp_process<false>, dim3(n), dim3(64), 0, st, pa);
}

}  // namespace lra_sdp

// lra_amd/csrc/sdp.hip -- SURVEY §8a row a8: the first sparse dynamic program of the low-accuracy path (SDP#A),
// SparseDP(vector<Cluster>&, vector<UltimateChain>&, ...) (SparseDP.h:2139-2279, called at Map_lowacc.h:188), for a
// whole batch of reads.  gfx950 only.
//
// What the reference does per read: every anchor becomes a start/end point pair per orientation family
// (insertPointsPair :79), the points are std::sort'ed by row and by column, four divide-and-conquer decompositions
// (DivideSubProbBy{Row,Col}{1,2}) build a tree of sub-problems holding the distinct diagonals of the end points of
// one half (Di) and of the start points of the other half (Ei); ProcessPoint (:1015) then walks the points in row
// order: a start point queries every sub-problem on its root-to-leaf paths (Maximization / FindValueInBlock, a
// candidate-list structure over the PWL gap cost, SubRountine.h:270-345), an end point deposits the anchor's value
// in them (PassValueToD*).  The result depends on the order of all these steps (values deposited after a
// candidate was consumed stay invisible, `last` moves backwards, slots are overwritten), so it is reproduced
// literally; what is re-designed is how it is laid out and scheduled:
//
//  * points, sorts: one thread per cluster writes the points; the two std::sorts are the library's libstdc++-exact
//    workgroup sort (exact_sort.hip) on packed 63-bit keys (q,t,ind / t,q,ind) -- the permutation of tied points is part
//    of the result because it fixes the processing order;
//  * decompositions: the sub-problem numbering is internal to the reference (prev_sub is only an index), so the trees
//    are built level by level instead of depth first: per family the points are kept sorted by diagonal and stably
//    partitioned by half at every level (prefix sums), which yields every node's sorted distinct Di/Ei at once;
//    Db/Eb have closed forms (counts of smaller diagonals), and every (point, level) gets its sub-problem and its
//    index in Di/Ei recorded -- the Lower_Bound searches of ProcessPoint/PassValueToD* disappear.  The records are kept
//    level by level: per read one plane of P records for every (family pair, level) it can have, vis[plane][point]
//    (sdp.h, ReadArena) -- a level of the build writes one plane, a lane of ProcessPoint streams along its own;
//  * ProcessPoint: one wave per read; lane (family pair, level) < 2 * LV owns the sub-problems of that level, so the sub-problems a
//    point touches advance concurrently and none is ever touched by two lanes; short candidate insertions run per lane, long ones
//    wave-cooperatively (prefetched candidates, iterations that change nothing skipped with a ballot, six-level probes in the
//    boundary search); the ordered `<` update of Value[ii] becomes a (max value, first in order) reduction; stacks / Block lists that
//    fill up double out of a per-read pool;
//  * TraceBack / DecidePrimaryChains: one lane per read after the exact sort of the values.
//
// Roofline: integer/float bookkeeping with dependent loads, HBM-nominal; algorithmic bytes = 44 B per sub-problem entry + 8 B per level of the read
// and family pair + 13 B per point (visit records + coordinates).  A launch lasts as long as its largest reads: one chunk per batch, largest first.
//
// This file is the driver: sdp_run, a sequence of named stages over the state of one call (lra_sdp::Call, sdp.h), and the two entry points.  The kernels and their
// launch functions are in sdp_points.hip, sdp_build.hip, sdp_process.hip, sdp_process_wg.hip and sdp_trace.hip, the analysis hooks in sdp_diag.hip (sdp.h lists them).
#include "sdp.h"
#include "scan.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <vector>

using namespace lra_sdp;

namespace {

inline size_t sz(size_t n, size_t elem) { return (n * elem + 255) / 256 * 256; }
inline char* take(char*& w, size_t n, size_t e) { char* p = w; w += sz(n, e); return p; }
#define SDP_TRY(call) do { const int rc__ = (call); if (rc__) return rc__; } while (0)

// from how many points on a read gets a workgroup (the workgroup kernels' per-point latency is half the wave kernel's, at four times its wave slots): a launch is as long
// as its largest reads' chains.  LRA_SDP_BIG_POINTS overrides it
static long sdp_big_points(const lra_ctx* ctx, int mode) {
  if (const char* e = getenv("LRA_SDP_BIG_POINTS")) return atol(e);
  if (ctx->sdp_inner) return 1500;
  if (mode == 0) return 2500;   // (its largest reads have ~5000 points: the top few hundred as workgroups, 93 -> 83 ms)
  // Two-stage batches: the other half of another batch fills what a long tail leaves idle, and a wave per read costs a third of the device time per point that a
  // workgroup per read does -- so only the reads that would make the wave launch far longer than everything beside it stay workgroup jobs (measured, two-stage step:
  // 6000: 980 ms, 9000: 954, 12000: 943, 14000: 933, 16000+: up again; each with at most one job per CU, see maxBig)
  return ctx->pipelined ? 14000 : 6000;
}

// InitPWL on the host (SubRountine.h:43-99), host libm as in the reference; -w as a table for small distances (the kernels copy it to LDS), left out when a penalty
// does not fit 16 bits
int pwl_table(Call& c) {
  lra_ctx* ctx = c.ctx; hipStream_t st = c.st; const lra_sdp_opts* opts = c.opts; PwlTab& pw = c.pw;
  {
    static const long long stv[25] = {0,    5,    10,   20,   40,   80,    100,   200,   300,   500,   1000,  2000, 3000,
                                      4000, 5000, 6000, 7000, 8000, 9000, 15000, 20000, 30000, 40000, 50000, 100000};
    float intercept = opts->gapopen, scalar = opts->gapextend, root = opts->gaproot, vals[25];
    for (int i = 0; i < 25; i++) { pw.stops[i] = stv[i]; pw.slope[i] = 0; pw.inter[i] = 0; }
    vals[0] = 0;
    for (int i = 1; i < 25; i++) { if (i <= 2) intercept = 0; vals[i] = intercept + scalar * std::pow((float)stv[i], 1 / root); }
    for (int i = 0; i < 24; i++) {
      float slope = (vals[i + 1] - vals[i]) / (stv[i + 1] - stv[i]);
      if (stv[i] <= 10) { pw.slope[i] = 0; pw.inter[i] = 0; }
      else { pw.slope[i] = slope; pw.inter[i] = vals[i] - stv[i] * slope + intercept; }
    }
    pw.c1 = opts->gapCeiling1; pw.c2 = opts->gapCeiling2;
  }
  c.d_penTab = (short*)lra_ensure(ctx, 190, PEN_TAB_WG * sizeof(short) + 64);
  c.penN = 0;
  if (c.d_penTab) {
    int* d_bad = (int*)(c.d_penTab + PEN_TAB_WG);
    LRA_HIP_CHECK(ctx, hipMemsetAsync(d_bad, 0, 4, st));
    launch_pen_table(st, pw, c.d_penTab, d_bad);
    int h_bad = 1;
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (!h_bad) c.penN = PEN_TAB_WG;
  }
  return LRA_OK;
}

// The batch's buffers -- clusters and reads (slot 7), fragments (slot 8), points (slot 9) -- with the counts and offsets that size them
int batch_buffers(Call& c) {
  lra_ctx* ctx = c.ctx; hipStream_t st = c.st; const lra_sdp_opts* opts = c.opts; lra_chain_result* out = c.out;
  const int n_reads = c.n_reads; const size_t n1 = c.n1;
  c.h_off.resize(n1);
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(c.h_off.data(), c.d_cluster_off, n1 * 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  const uint64_t NC = c.NC = c.h_off[n_reads];
  // ---- batch-level buffers: clusters and reads
  const size_t nslot = c.nslot = (size_t)n_reads * opts->NumAln;
  size_t needA = sz(NC + 1, 4) * 3 + sz(NC + 2, 8) * 2 + sz(n1, 8) * 2 + sz(n1, 4) * 2 + sz(nslot, 8) + sz(nslot, 4) * 3 + sz(4 * nslot, 4) + 4096;
  char* wa = (char*)lra_ensure(ctx, 7, needA);
  if (!wa) return LRA_ERR_NOMEM;
  c.clusFragCnt = (uint32_t*)take(wa, NC + 1, 4); c.clusPtCnt = (uint32_t*)take(wa, NC + 1, 4); c.clusRead = (uint32_t*)take(wa, NC + 1, 4);
  c.clusFragOff = (uint64_t*)take(wa, NC + 2, 8); c.clusPtOff = (uint64_t*)take(wa, NC + 2, 8);
  c.fragOff = (uint64_t*)take(wa, n1, 8); c.ptOff = (uint64_t*)take(wa, n1, 8);
  c.status = (uint32_t*)take(wa, n1, 4); c.nChains = (uint32_t*)take(wa, n1, 4);
  c.chainStart = (uint64_t*)take(wa, nslot, 8); c.chainLen = (uint32_t*)take(wa, nslot, 4); c.chainValue = (float*)take(wa, nslot, 4);
  c.chainBox = (uint32_t*)take(wa, 4 * nslot, 4);
  c.chainNum = (int32_t*)take(wa, nslot, 4);
  LRA_HIP_CHECK(ctx, hipMemsetAsync(c.chainLen, 0, nslot * 4, st));
  if (NC > 0) {
    lra_time_begin(ctx, ctx->sdp_inner ? "sdp_inner_points" : "sdp_points");
    launch_cluster_counts(st, NC, c.boxes ? nullptr : c.d_c_count, c.clusFragCnt, c.clusPtCnt, opts->mode == LRA_SDP_SINGLE_CLUSTER);
    lra_time_end(ctx);
  }
  SDP_TRY(lra_exclusive_scan<uint32_t>(ctx, (long)NC, c.clusFragCnt, c.clusFragOff));
  SDP_TRY(lra_exclusive_scan<uint32_t>(ctx, (long)NC, c.clusPtCnt, c.clusPtOff));
  launch_read_offsets(st, n_reads, c.d_cluster_off, c.clusFragOff, c.clusPtOff, c.fragOff, c.ptOff, c.clusRead, c.status, c.nChains);
  c.h_frag.resize(n1); c.h_pt.resize(n1);
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(c.h_frag.data(), c.fragOff, n1 * 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(c.h_pt.data(), c.ptOff, n1 * 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  const uint64_t NF = c.NF = c.h_frag[n_reads], NP = c.NP = c.h_pt[n_reads];
  out->n_frags = NF; out->n_points = NP;
  // ---- fragments
  size_t needF = sz(NF + 1, 4) * 16 + sz(2 * NF + 2, 4) + sz(NF + 1, 1) * 5 + sz(NF + 1, 8) * 2 + 4096;
  char* wf = (char*)lra_ensure(ctx, 8, needF);
  if (!wf) return LRA_ERR_NOMEM;
  c.fq = (uint32_t*)take(wf, NF + 1, 4); c.ft = (uint32_t*)take(wf, NF + 1, 4); c.flen = (int32_t*)take(wf, NF + 1, 4);
  c.fcl = (uint32_t*)take(wf, NF + 1, 4); c.fai = (uint32_t*)take(wf, NF + 1, 4); c.fval = (float*)take(wf, NF + 1, 4);
  c.fprevNode = (uint32_t*)take(wf, NF + 1, 4); c.fprevInd = (uint32_t*)take(wf, NF + 1, 4);
  c.ccl = (uint32_t*)take(wf, NF + 1, 4); c.can = (uint32_t*)take(wf, NF + 1, 4);
  c.fflags = (uint8_t*)take(wf, NF + 1, 1); c.used = (uint8_t*)take(wf, NF + 1, 1); c.clink = (uint8_t*)take(wf, NF + 1, 1);
  c.fstrand = (uint8_t*)take(wf, NF + 1, 1); c.cstrand = (uint8_t*)take(wf, NF + 1, 1);
  c.cq = (uint32_t*)take(wf, NF + 1, 4); c.ct = (uint32_t*)take(wf, NF + 1, 4); c.clen = (int32_t*)take(wf, NF + 1, 4);
  c.okey = (uint64_t*)take(wf, NF + 1, 8);
  c.fqe = (uint32_t*)take(wf, NF + 1, 4); c.fte = (uint32_t*)take(wf, NF + 1, 4);
  // ---- points
  size_t needP = sz(NP + 1, 8) * 3 + sz(NP + 1, 4) * 11 + sz(NP + 1, 1) * 2 + sz(NF + 1, 4) * 2 + 4096;
  char* wp = (char*)lra_ensure(ctx, 9, needP);
  if (!wp) return LRA_ERR_NOMEM;
  c.key1 = (uint64_t*)take(wp, NP + 1, 8); c.key2 = (uint64_t*)take(wp, NP + 1, 8); c.key3 = (uint64_t*)take(wp, NP + 1, 8);
  c.pay1 = (uint32_t*)take(wp, NP + 1, 4); c.pay2 = (uint32_t*)take(wp, NP + 1, 4); c.pay3 = (uint32_t*)take(wp, NP + 1, 4);
  c.iq = (uint32_t*)take(wp, NP + 1, 4); c.it = (uint32_t*)take(wp, NP + 1, 4); c.ifr = (uint32_t*)take(wp, NP + 1, 4);
  c.ptRead = (uint32_t*)take(wp, NP + 1, 4);
  c.hq = (uint32_t*)take(wp, NP + 1, 4); c.ht = (uint32_t*)take(wp, NP + 1, 4); c.hfr = (uint32_t*)take(wp, NP + 1, 4);
  c.spare = (uint32_t*)take(wp, NP + 1, 4);          // TraceBack's predecessor per fragment (k_pred)
  c.ifl = (uint8_t*)take(wp, NP + 1, 1); c.hfl = (uint8_t*)take(wp, NP + 1, 1);
  c.opay = (uint32_t*)take(wp, NF + 1, 4); c.fragRead = (uint32_t*)take(wp, NF + 1, 4);
  out->d_n_chains = c.nChains; out->d_chain_start = c.chainStart; out->d_chain_len = c.chainLen; out->d_chain_box = c.chainBox; out->d_chain_value = c.chainValue;
  out->d_chain_cluster = c.ccl; out->d_chain_anchor = c.can; out->d_chain_link = c.clink; out->d_chain_q = c.cq; out->d_chain_t = c.ct; out->d_chain_alen = c.clen;
  out->d_chain_strand = c.cstrand; out->d_frag_off = c.fragOff; out->d_frag_val = c.fval; out->d_status = c.status;
  out->d_chain_num_anchors = c.boxes ? c.chainNum : nullptr;
  return LRA_OK;
}

// anchors -> compact fragment arrays + points in insertion order; which read a fragment belongs to
void make_points(const Call& c) {
  lra_ctx* ctx = c.ctx; const lra_sdp_opts* opts = c.opts;
  PtArgs pa;
  pa.nc = c.NC; pa.cluster_off = c.d_cluster_off; pa.c_start = c.d_c_start; pa.c_count = c.d_c_count; pa.c_strand = c.d_c_strand; pa.q = c.d_q; pa.t = c.d_t; pa.len = c.d_len;
  pa.clusRead = c.clusRead; pa.clusFragOff = c.clusFragOff; pa.clusPtOff = c.clusPtOff; pa.fragOff = c.fragOff; pa.ptOff = c.ptOff; pa.rate_in = c.d_rate; pa.rate = opts->rate; pa.single = opts->mode == LRA_SDP_SINGLE_CLUSTER;
  pa.fq = c.fq; pa.ft = c.ft; pa.flen = c.flen; pa.fcl = c.fcl; pa.fai = c.fai; pa.fval = c.fval; pa.fprevNode = c.fprevNode; pa.fprevInd = c.fprevInd; pa.fflags = c.fflags; pa.used = c.used; pa.fstrand = c.fstrand;
  pa.qe = c.d_qe; pa.te = c.d_te; pa.fqe = c.fqe; pa.fte = c.fte;
  pa.key1 = c.key1; pa.pay1 = c.pay1; pa.iq = c.iq; pa.it = c.it; pa.ifl = c.ifl; pa.ifr = c.ifr; pa.ptRead = c.ptRead;
  lra_time_begin(ctx, ctx->sdp_inner ? "sdp_inner_points" : "sdp_points");
  launch_points(c.st, pa);
  launch_frag_read(c.st, c.n_reads, c.fragOff, c.fragRead);
  lra_time_end(ctx);
}

// The three point orders: by row (H1), by column (H2), by diagonal per point class
int sort_points(const Call& c) {
  lra_ctx* ctx = c.ctx; hipStream_t st = c.st; const int n_reads = c.n_reads; const uint64_t NP = c.NP;
  // the two point orders: (q, t, ind) / (t, q, ind) keys repeat only where two anchors share a corner, so the radix path takes nearly all lists
  SDP_TRY(lra_sort_mostly_unique_batch(ctx, n_reads, c.ptOff, NP, c.key1, c.pay1, c.key3, c.pay3, 64, c.sort));   // sort(H1, SortByRowOp)  :2171
  lra_time_begin(ctx, ctx->sdp_inner ? "sdp_inner_points" : "sdp_points");
  // after the row sort: the point attributes in H1 order, the column-sort and diagonal-sort keys
  launch_gather(st, NP, c.ptRead, c.ptOff, c.pay1, c.iq, c.it, c.ifl, c.ifr, c.hq, c.ht, c.hfl, c.hfr, c.key2, c.pay2, c.key3, c.pay3);
  lra_time_end(ctx);
  SDP_TRY(lra_sort_mostly_unique_batch(ctx, n_reads, c.ptOff, NP, c.key2, c.pay2, c.key1, c.pay1, 63, c.sort));   // sort(H2, SortByColOp)  :2174
  // diagonal order per point class: any sorted order serves (ties are the same diagonal), so this one is a segmented radix sort -- the
  // exact introsort degenerates on the long runs of equal diagonals.  Sorted into the (now free) key1 / pay1 buffers.
  lra_time_begin(ctx, c.sort.tag);
  const int rc = lra_segsort_pairs_scratch(ctx, c.key3, c.key1, c.pay3, c.pay1, NP, (uint64_t)n_reads, c.ptOff, c.ptOff + 1, 0, 42);
  lra_time_end(ctx);
  if (rc) return rc;
  LRA_HIP_CHECK(ctx, hipGetLastError());
  return LRA_OK;
}

// ---- per chunk of reads
// The chunk's work buffers (slot 10) and its reads' order, largest first
int chunk_begin(const Call& c, Chunk& k) {
  lra_ctx* ctx = c.ctx; hipStream_t st = c.st; const std::vector<uint64_t>& h_pt = c.h_pt;
  const int r0 = k.r0, nr = k.nr; const uint64_t cp = k.cp;
  const size_t nr1 = (size_t)nr + 1;
  size_t needS = sz(34 * cp + 64 * (size_t)nr + 64, 4) + sz(nr1, 4) * 8 + sz(2 * nr1, 4) + sz(nr1 + 1, 8) * 3 + sz(nr1, sizeof(ReadArena)) + 4096;
  char* ws = (char*)lra_ensure(ctx, 10, needS);
  if (!ws) return LRA_ERR_NOMEM;
  k.scratch = (uint32_t*)take(ws, 34 * cp + 64 * (size_t)nr + 64, 4);
  k.cntE = (uint32_t*)take(ws, nr1, 4); k.cntN = (uint32_t*)take(ws, nr1, 4); k.cntD = (uint32_t*)take(ws, nr1, 4);
  k.cntV = (uint32_t*)take(ws, nr1, 4); k.cntRC = (uint32_t*)take(ws, nr1, 4); k.order = (uint32_t*)take(ws, nr1, 4); k.order2 = (uint32_t*)take(ws, nr1, 4); k.poolUsed = (uint32_t*)take(ws, nr1, 4);
  k.lines = (uint32_t*)take(ws, 2 * nr1, 4);
  LRA_HIP_CHECK(ctx, hipMemsetAsync(k.lines, 0, 2 * nr1 * 4, st));             // (no read's rows / columns counted yet)
  {
    // largest first, equal sizes in read order: a counting sort by size (a13's inner sparse DP orders 170 k jobs: 11 ms of std::sort with the device idle)
    std::vector<uint32_t> h_order(nr);
    uint64_t maxP = 0;
    for (int i = 0; i < nr; i++) maxP = std::max<uint64_t>(maxP, h_pt[r0 + i + 1] - h_pt[r0 + i]);
    if (maxP <= (uint64_t(1) << 24)) {
      std::vector<uint32_t> at(maxP + 2, 0);
      for (int i = 0; i < nr; i++) at[maxP - (h_pt[r0 + i + 1] - h_pt[r0 + i]) + 1]++;
      for (uint64_t v = 1; v <= maxP + 1; v++) at[v] += at[v - 1];
      for (int i = 0; i < nr; i++) h_order[at[maxP - (h_pt[r0 + i + 1] - h_pt[r0 + i])]++] = (uint32_t)i;
    } else {
      for (int i = 0; i < nr; i++) h_order[i] = (uint32_t)i;
      std::sort(h_order.begin(), h_order.end(), [&](uint32_t x, uint32_t y) {
        const uint64_t px = h_pt[r0 + x + 1] - h_pt[r0 + x], py = h_pt[r0 + y + 1] - h_pt[r0 + y];
        return px != py ? px > py : x < y;
      });
    }
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(k.order, h_order.data(), (size_t)nr * 4, hipMemcpyHostToDevice, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    k.h_orderAll = h_order;
  }
  take(ws, nr1 + 1, 8);                                                     // (room of a table no longer kept: the layout stays as it is)
  k.bytes = (uint64_t*)take(ws, nr1 + 1, 8); k.byteOff = (uint64_t*)take(ws, nr1 + 1, 8);
  k.ra = (ReadArena*)take(ws, nr1, sizeof(ReadArena));
  BuildArgs& ba = k.ba;
  memset(&ba, 0, sizeof ba);
  ba.r0 = r0; ba.n = nr; ba.ptOff = c.ptOff; ba.hq = c.hq; ba.ht = c.ht; ba.hfl = c.hfl; ba.h2 = c.pay2; ba.key3 = c.key1; ba.pay3 = c.pay1; ba.scratch = k.scratch;
  ba.cntEntries = k.cntE; ba.cntNodes = k.cntN; ba.cntD = k.cntD; ba.cntV = k.cntV; ba.cntRC = k.cntRC; ba.lines = k.lines; ba.status = c.status; ba.order = k.order; ba.stat = nullptr;
  if (diag_build_stat()) { k.buildStat.alloc(16, st); ba.stat = k.buildStat.d; }
  k.h_status.assign(nr, 0);
  k.subOrder = k.order; k.nsub = nr;
  return LRA_OK;
}

// The count pass over reads d_ord / h_ord [0, n): the same divide as the emit pass, for the sizes of a read's blocks
void count_pass(const Call& c, const Chunk& k, const uint32_t* d_ord, const std::vector<uint32_t>& h_ord, int n) {
  lra_ctx* ctx = c.ctx; hipStream_t st = c.st; const lra_sdp_opts* opts = c.opts; const std::vector<uint64_t>& h_pt = c.h_pt; const int r0 = k.r0;
  lra_time_begin(ctx, ctx->sdp_inner ? "sdp_inner_build_count" : "sdp_build_count");
  // reads ordered largest first: the large ones get a 1024-thread workgroup each, beside the wave-per-read launch
  const long big_pts = sdp_big_points(ctx, opts->mode);
  int nb0 = 0;
  while (nb0 < n && (long)(h_pt[r0 + h_ord[nb0] + 1] - h_pt[r0 + h_ord[nb0]]) >= big_pts) nb0++;
  const bool forked = nb0 > 0 && n > nb0;
  BuildArgs bc = k.ba; bc.order = d_ord; bc.n = n;
  if (nb0 > 0) launch_wg_builds(false, forked ? lra_side_fork(ctx) : st, bc, nb0);
  if (n > nb0) launch_small_builds(false, ctx, bc, d_ord, h_ord, h_pt.data() + r0, nb0, n);
  if (forked) lra_side_join(ctx);
  lra_time_end(ctx);
}

// max(rows, columns) over the chunk's reads and the entries the reads have (the count pass's cntE, or what the emit pass found: cntV)
int read_rc(const Call& c, Chunk& k) {
  lra_ctx* ctx = c.ctx; hipStream_t st = c.st; const int nr = k.nr;
  std::vector<uint32_t> h_rc(nr), h_e(nr);
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(h_rc.data(), k.cntRC, (size_t)nr * 4, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(h_e.data(), k.onePass ? k.cntV : k.cntE, (size_t)nr * 4, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  k.maxRC = 0; k.totE = 0;
  for (uint32_t v : h_rc) k.maxRC = std::max(k.maxRC, v);
  for (uint32_t v : h_e) k.totE += v;
  return LRA_OK;
}

// The sizes of the reads' blocks: the count pass for everything only on request (LRA_SDP_ONEPASS=0, LRA_SDP_RATIOS); otherwise the blocks are laid out from
// k_arena_estimate and only the reads that outgrow them are counted (attempt 1)
int chunk_sizes(const Call& c, Chunk& k) {
  const lra_sdp_opts* opts = c.opts; const int nr = k.nr;
  const bool onePassEnv = !(getenv("LRA_SDP_ONEPASS") && getenv("LRA_SDP_ONEPASS")[0] == '0');
  k.onePass = onePassEnv && !getenv("LRA_SDP_RATIOS");
  if (!k.onePass) { count_pass(c, k, k.order, k.h_orderAll, nr); SDP_TRY(read_rc(c, k)); }
  else {
    float fE = opts->mode == 0 ? 10.0f : 8.5f, fN = 2.0f;
    if (const char* e = getenv("LRA_SDP_ESTIMATE")) { float x = 0, y = 0; if (sscanf(e, "%f,%f", &x, &y) == 2 && x > 0 && y > 0) { fE = x; fN = y; } }   // (tests: estimates that many reads outgrow)
    launch_arena_estimate(c.st, nr, k.r0, c.ptOff, fE, fN, k.cntE, k.cntN, k.cntD);
  }
  diag_ratios(c, k);
  return LRA_OK;
}

// ---- one attempt: the build and ProcessPoint of the reads k.subOrder[0, k.nsub)
// Which reads of the attempt get a workgroup each (they are ordered by their number of points, largest first), and whether those go first
void pick_large_reads(const Call& c, const Chunk& k, Attempt& a) {
  lra_ctx* ctx = c.ctx; const lra_sdp_opts* opts = c.opts; const std::vector<uint64_t>& h_pt = c.h_pt; const std::vector<uint32_t>& ordAtt = *a.ordAtt;
  const int r0 = k.r0, nsub = k.nsub, att = a.att; const bool onePass = k.onePass, dbg = a.dbg;
  int nbig = 0;
  {
    const long big_pts = sdp_big_points(ctx, opts->mode);   // (tests lower it to run small reads through the workgroup kernels)
    // ... but no more of them than the device runs side by side (a workgroup holds 16 wave slots for a per-point latency a third of the wave kernel's, at 3.5 times its
    // wave-time per point): beyond that the large reads queue up behind each other, and the ones further down the order are better off as one wave each
    // (two-stage batches: one round of workgroup jobs -- one per CU, all resident at once; 192: 1026 ms, 256: 933, 320: 955)
    const int maxBigAll = ctx->pipelined ? ctx->num_cu : (1 << 30);
    const int maxBig = (opts->mode == 0 && !ctx->sdp_inner) ? std::min(maxBigAll, 512) : maxBigAll;
    while (nbig < nsub && nbig < maxBig && (long)(h_pt[r0 + ordAtt[nbig] + 1] - h_pt[r0 + ordAtt[nbig]]) >= big_pts) nbig++;
  }
  const bool forked = nbig > 0 && nsub > nbig;
  // LARGE READS FIRST (attempt 0, LRA_SDP_BIG_FIRST=0 switches it off).  The stage is as long as the chain build -> ProcessPoint of its largest read, and that read is one
  // of the workgroup jobs: their build goes first, on the side stream, with nothing of this stage beside it; their ProcessPoint launch follows it on that stream at
  // once -- what it needs from the host (the per-anchor words' offsets, the kernel variant) is made ready before the builds: the variant from the large reads' own rows /
  // columns (k_big_lines) instead of the emit pass's counts --; the small reads' builds start behind the large reads' build and their wave-per-read ProcessPoint launch
  // behind those, beside the workgroup launch as before.  What used to be  max(builds) + max(ProcessPoint launches)  is  build_large + max(wg, builds_small + wave).
  const bool bigFirstEnv = !(getenv("LRA_SDP_BIG_FIRST") && getenv("LRA_SDP_BIG_FIRST")[0] == '0');   // (read per call: the tests run both orders in one process)
  const bool early = bigFirstEnv && att == 0 && onePass && forked && !dbg;
  a.nbig = nbig; a.forked = forked; a.early = early;
}

// The large reads' per-anchor words (see sdp_process_wg) and the reads' arenas, sized on the device.  It queues a copy out of k.woff and copies into a.totB / a.bigLines
// and waits for none of them: the caller does, on every way out of here.
int arena_layout(const Call& c, Chunk& k, Attempt& a) {
  lra_ctx* ctx = c.ctx; hipStream_t st = c.st; const std::vector<uint64_t>& h_frag = c.h_frag; const std::vector<uint64_t>& h_pt = c.h_pt;
  const std::vector<uint32_t>& ordAtt = *a.ordAtt; std::vector<uint64_t>& woff = k.woff;
  const int r0 = k.r0, nsub = k.nsub, nbig = a.nbig;
  woff.assign((size_t)nbig + 1, 0);
  if (nbig > 0) {
    for (int i = 0; i < nbig; i++) {
      const uint64_t rdx = (uint64_t)r0 + ordAtt[i];
      const uint64_t Fr = h_frag[rdx + 1] - h_frag[rdx], Pr = h_pt[rdx + 1] - h_pt[rdx];
      woff[i + 1] = woff[i] + ((36 * Fr + 4 * Pr + 64 + 8 + 256 * 8 + 255) & ~(uint64_t)255);
    }
    a.wsc = (char*)lra_ensure(ctx, 177, woff[nbig] + 256);
    a.dwoff = (uint64_t*)lra_ensure(ctx, 178, ((size_t)nbig + 4) * 8);
    if (!a.wsc || !a.dwoff) return LRA_ERR_NOMEM;
    a.d_maxLines = (uint32_t*)(a.dwoff + nbig + 2);
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(a.dwoff, woff.data(), ((size_t)nbig + 1) * 8, hipMemcpyHostToDevice, st));
    if (a.early) {
      LRA_HIP_CHECK(ctx, hipMemsetAsync(a.d_maxLines, 0, 4, st));
      launch_big_lines(st, nbig, r0, k.subOrder, c.ptOff, c.hq, c.ht, c.pay2, a.d_maxLines, k.lines);
    }
  }
  launch_arena_sizes(st, nsub, r0, c.ptOff, k.cntE, k.cntN, k.cntD, k.lines, k.ra, k.bytes, k.subOrder, a.shift);
  SDP_TRY(lra_exclusive_scan<uint64_t>(ctx, nsub, k.bytes, k.byteOff));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&a.totB, k.byteOff + nsub, 8, hipMemcpyDeviceToHost, st));
  if (a.early) LRA_HIP_CHECK(ctx, hipMemcpyAsync(&a.bigLines, a.d_maxLines, 4, hipMemcpyDeviceToHost, st));
  return LRA_OK;
}

// The emit pass.  LARGE READS FIRST (a.early): see pick_large_reads
int emit_builds(const Call& c, Chunk& k, Attempt& a) {
  lra_ctx* ctx = c.ctx; hipStream_t st = c.st; const std::vector<uint32_t>& ordAtt = *a.ordAtt; BuildArgs& ba = k.ba;
  const uint64_t* h_pt0 = c.h_pt.data() + k.r0;
  const int nsub = k.nsub, nbig = a.nbig;
  if (a.early) LRA_HIP_CHECK(ctx, hipMemsetAsync(k.poolUsed, 0, (size_t)k.nr * 4, st));   // (in front of the fork: the workgroup launch uses its reads' pools)
  lra_time_begin(ctx, ctx->sdp_inner ? "sdp_inner_build" : "sdp_build");
  launch_visit_clear(st, nsub, k.ra, k.byteOff, k.subOrder);
  ba.ra = k.ra; ba.order = k.subOrder;
  if (a.early) {
    hipStream_t ws = lra_side_fork(ctx);
    if (ws == st) {                                                  // (no side stream: the old order, everything on the one stream)
      launch_wg_builds(true, st, ba, nbig);
      launch_small_builds(true, ctx, ba, k.subOrder, ordAtt, h_pt0, nbig, nsub);
      launch_process_wg(st, a.pa, nbig, a.bigLines, a.dbg);
    } else {
      launch_wg_builds(true, ws, ba, nbig);
      // the small reads' builds behind the large reads' build (an event of its own: the join event is the end of the workgroup ProcessPoint launch)
      if (!ctx->ev_mid) (void)hipEventCreateWithFlags(&ctx->ev_mid, hipEventDisableTiming);
      if (ctx->ev_mid) { (void)hipEventRecord(ctx->ev_mid, ws); (void)hipStreamWaitEvent(st, ctx->ev_mid, 0); }
      lra_time_begin(ctx, ctx->sdp_inner ? "sdp_inner_process_wg" : "sdp_process_wg", ws);
      launch_process_wg(ws, a.pa, nbig, a.bigLines, a.dbg);
      lra_time_end(ctx, ws);
      launch_small_builds(true, ctx, ba, k.subOrder, ordAtt, h_pt0, nbig, nsub);
    }
  } else {
    if (nbig > 0) launch_wg_builds(true, a.forked ? lra_side_fork(ctx) : st, ba, nbig);
    if (nsub > nbig) launch_small_builds(true, ctx, ba, k.subOrder, ordAtt, h_pt0, nbig, nsub);
    if (a.forked) lra_side_join(ctx);
  }
  lra_time_end(ctx);
  if (k.onePass && a.att == 0) SDP_TRY(read_rc(c, k));                  // (rows / columns of the reads, known after the emit pass only)
  return LRA_OK;
}

// ProcessPoint: the few large reads (a workgroup each) run beside the many small ones (a wave each) instead of in front of them
int process_points(const Call& c, Chunk& k, Attempt& a) {
  lra_ctx* ctx = c.ctx; hipStream_t st = c.st;
  const int nsub = k.nsub, nbig = a.nbig;
  if (a.att > 0)
    launch_reset_frags(st, nsub, k.r0, k.subOrder, c.fragOff, c.flen, c.d_rate, c.opts->rate, c.fval, c.fprevNode, c.fprevInd, c.fflags, c.status);
  if (!a.early) LRA_HIP_CHECK(ctx, hipMemsetAsync(k.poolUsed, 0, (size_t)k.nr * 4, st));
  diag_dbg_begin(c, a);
  lra_time_begin(ctx, ctx->sdp_inner ? "sdp_inner_process" : "sdp_process");
  if (nbig > 0 && !a.early) launch_process_wg(a.forked ? lra_side_fork(ctx) : st, a.pa, nbig, k.maxRC, a.dbg);
  const int statEnv = diag_stat_level();
  StatBuf stat;                                                            // (LRA_SDP_STAT)
  if (nsub > nbig) {
    ProcArgs pb = a.pa; pb.order = k.subOrder + nbig; pb.n = nsub - nbig; pb.stat = nullptr;
    if (statEnv > 0) stat.alloc(40, st);
    if (stat.d) { pb.stat = stat.d; pb.dbg = statEnv; }
    launch_process(st, pb, nsub - nbig, stat.d != nullptr);
  }
  if (a.forked) lra_side_join(ctx);
  lra_time_end(ctx);
  diag_stat(c, a, nsub - nbig, stat);
  diag_dbg_end(c, k, a);
  return LRA_OK;
}

// The reads whose candidate stack / Block (or whose estimated blocks) ran out: the next attempt's
int collect_outgrown(const Call& c, Chunk& k, const Attempt& a) {
  lra_ctx* ctx = c.ctx; hipStream_t st = c.st; const int nr = k.nr;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(k.h_status.data(), c.status + k.r0, (size_t)nr * 4, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  k.h_sub.clear();
  for (int i = 0; i < k.nsub; i++) { const uint32_t rr = (*a.ordAtt)[i]; if (k.h_status[rr] & LRA_ST_CAPACITY) k.h_sub.push_back(rr); }
  k.nsub = (int)k.h_sub.size();
  if (k.nsub == 0) return LRA_OK;
  k.h_prev = k.h_sub;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(k.order2, k.h_sub.data(), (size_t)k.nsub * 4, hipMemcpyHostToDevice, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  k.subOrder = k.order2;
  return LRA_OK;
}

// attempt 0: all reads of the chunk; attempts 1, 2: the reads whose candidate stack / Block outgrew its slots, with 8x / 64x the slots
int attempt(const Call& c, Chunk& k, int att) {
  lra_ctx* ctx = c.ctx; hipStream_t st = c.st;
  Attempt a;
  a.att = att; a.shift = 3 * att; a.slot = att == 0 ? 12 : 21 + att;
  if (k.onePass && att == 1) count_pass(c, k, k.subOrder, k.h_prev, k.nsub);   // (exact sizes for the reads that come back: some outgrew their estimated blocks)
  a.dbg = diag_dbg();
  a.ordAtt = att == 0 ? &k.h_orderAll : &k.h_prev;
  pick_large_reads(c, k, a);
  {
    const int rc = arena_layout(c, k, a);
    const hipError_t e = hipStreamSynchronize(st);                         // the one wait behind the copies arena_layout queued, whichever way it ended
    if (rc) return rc;
    LRA_HIP_CHECK(ctx, e);
  }
  char* arena = (char*)lra_ensure(ctx, a.slot, a.totB + 4096);
  if (!arena) return LRA_ERR_NOMEM;
  launch_arena_bases(st, k.nsub, k.byteOff, k.ra, k.subOrder, arena);
  ProcArgs& pa = a.pa;
  pa.wgScratch = a.wsc; pa.wgOff = a.dwoff; pa.dbg = (a.dbg && a.nbig > 0) ? 1 : 0; { const char* e = getenv("LRA_SDP_WG_RING"); pa.wgNoRing = (e && e[0] == '0') ? 1 : 0; }
  if (a.nbig > 0) {
    const uint64_t rd0 = (uint64_t)k.r0 + (*a.ordAtt)[0];
    a.dbgOff0 = k.woff[0] + 36 * (c.h_frag[rd0 + 1] - c.h_frag[rd0]) + 4 * (c.h_pt[rd0 + 1] - c.h_pt[rd0]); a.dbgBase = a.wsc;
  }
  pa.r0 = k.r0; pa.n = k.nsub; pa.order = k.subOrder; pa.ptOff = c.ptOff; pa.fragOff = c.fragOff; pa.hfl = c.hfl; pa.hfr = c.hfr; pa.flen = c.flen; pa.fval = c.fval;
  pa.fprevNode = c.fprevNode; pa.fprevInd = c.fprevInd; pa.fflags = c.fflags; pa.rate_in = c.d_rate; pa.rate = c.opts->rate; pa.ra = k.ra;
  pa.status = c.status; pa.pwl = c.pw; pa.poolUsed = k.poolUsed; pa.penTab = c.d_penTab; pa.penN = c.penN;
  SDP_TRY(emit_builds(c, k, a));
  SDP_TRY(process_points(c, k, a));
  if (att == 2) return LRA_OK;
  return collect_outgrown(c, k, a);
}

// The value order, TraceBack, DecidePrimaryChains for the chunk's reads
int trace_chains(const Call& c, const Chunk& k) {
  lra_ctx* ctx = c.ctx; hipStream_t st = c.st; const lra_sdp_opts* opts = c.opts; const int r0 = k.r0, nr = k.nr;
  const uint64_t cf0 = c.h_frag[r0], cfn = c.h_frag[k.r1] - c.h_frag[r0];
  if (cfn == 0) return LRA_OK;
    lra_time_begin(ctx, ctx->sdp_inner ? "sdp_inner_trace" : "sdp_trace");
    // The value order (Fragment_valueOrder::Sort) is what DecidePrimaryChains walks; the single-cluster drivers (SparseDP.h:2417-2434, SparseDP_Forward.h) take the first
    // anchor of maximal value and nothing else of it: sdp_trace finds that anchor by a scan, so the keys and the exact sort are left out there (the second sparse DP of a
    // batch: 29 M values through the libstdc++-exact sort for nothing, 23 ms of the back half's chain)
    const bool needOrder = opts->mode != LRA_SDP_SINGLE_CLUSTER;
  if (needOrder) launch_valkeys(st, cf0, cfn, c.fval, c.fragRead, c.fragOff, c.okey, c.opay);
  launch_pred(st, cf0, cfn, r0, c.fragRead, c.fprevNode, c.fprevInd, c.status, k.ra, c.spare);
  lra_time_end(ctx);
  if (needOrder) SDP_TRY(lra_sort_exact_batch(ctx, nr, c.fragOff + r0, c.okey, c.opay, c.sort));   // Fragment_valueOrder::Sort (Fragment_Info.h:88)
  TraceArgs ta;
  ta.r0 = r0; ta.n = nr; ta.numAln = opts->NumAln; ta.single = opts->mode == LRA_SDP_SINGLE_CLUSTER; ta.alnthres = opts->alnthres; ta.fragOff = c.fragOff; ta.read_off = c.d_read_off; ta.fq = c.fq; ta.ft = c.ft;
  ta.flen = c.flen; ta.fcl = c.fcl; ta.fai = c.fai; ta.fval = c.fval; ta.fpred = c.spare; ta.fflags = c.fflags; ta.opay = c.opay; ta.used = c.used;
  ta.ra = k.ra; ta.nChains = c.nChains; ta.chainStart = c.chainStart; ta.chainLen = c.chainLen;
  ta.chainBox = c.chainBox; ta.chainValue = c.chainValue; ta.ccl = c.ccl; ta.can = c.can; ta.clink = c.clink; ta.status = c.status;
  ta.cq = c.cq; ta.ct = c.ct; ta.clen = c.clen; ta.cstrand = c.cstrand; ta.fstrand = c.fstrand;
  ta.boxes = c.boxes; ta.globalK = opts->globalK; ta.fqe = c.fqe; ta.fte = c.fte; ta.numAnchors = c.d_num_anchors; ta.chainNum = c.chainNum;
  lra_time_begin(ctx, ctx->sdp_inner ? "sdp_inner_trace" : "sdp_trace");
  launch_trace(st, ta);
  lra_time_end(ctx);
  return LRA_OK;
}

int sdp_run(lra_ctx* ctx, int n_reads, const uint64_t* d_cluster_off, const uint64_t* d_c_start, const uint32_t* d_c_count,
            const int32_t* d_c_strand, const uint32_t* d_q, const uint32_t* d_t, const int32_t* d_len, const uint64_t* d_read_off,
            const float* d_rate, const lra_sdp_opts* opts, lra_chain_result* out, const uint32_t* d_qe, const uint32_t* d_te,
            const int32_t* d_num_anchors) {
  if (!ctx || !out || !opts || n_reads < 0) return LRA_ERR_INVALID;
  if (opts->NumAln < 1 || opts->NumAln > MAXALN) return lra_set_err(ctx, LRA_ERR_INVALID, "NumAln must be 1..%d", MAXALN);
  memset(out, 0, sizeof *out);
  out->n_reads = n_reads; out->num_aln = opts->NumAln;
  if (n_reads == 0) return LRA_OK;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  Call c;
  c.ctx = ctx; c.st = ctx->stream; c.opts = opts; c.out = out; c.n_reads = n_reads; c.n1 = (size_t)n_reads + 1;
  c.d_cluster_off = d_cluster_off; c.d_c_start = d_c_start; c.d_c_count = d_c_count; c.d_c_strand = d_c_strand; c.d_q = d_q; c.d_t = d_t; c.d_len = d_len;
  c.d_read_off = d_read_off; c.d_rate = d_rate; c.d_qe = d_qe; c.d_te = d_te; c.d_num_anchors = d_num_anchors; c.boxes = d_qe != nullptr;
  c.sort = ctx->sdp_inner ? lra_sort_opts{"sdp_inner_sort", "sdp_inner_sort_fallback", true} : lra_sort_opts{"sdp_sort", "sdp_sort_fallback", true};
  SDP_TRY(pwl_table(c));
  SDP_TRY(batch_buffers(c));
  if (c.NF == 0) { LRA_HIP_CHECK(ctx, hipStreamSynchronize(c.st)); return LRA_OK; }
  make_points(c);
  SDP_TRY(diag_dump(c));
  SDP_TRY(sort_points(c));
  // ---- chunks of reads: decompositions, ProcessPoint, trace
  // one chunk if it fits: the kernels' duration is set by the longest read once the chip is no longer full, so few large launches
  // beat many small ones (32768 reads, sdp_process: 4 chunks 420 ms, 2 chunks 255 ms, 1 chunk 187 ms)
  constexpr uint64_t chunkPts = 96ull << 20;  // ~75 GB of arenas per chunk: a 32768-read batch of 30 kb reads (80 M points) is one chunk
  const std::vector<uint64_t>& h_pt = c.h_pt;
  for (int r0 = 0; r0 < n_reads;) {
    int r1 = r0 + 1;
    while (r1 < n_reads && h_pt[r1 + 1] - h_pt[r0] <= chunkPts) r1++;
    Chunk k;
    k.r0 = r0; k.r1 = r1; k.nr = r1 - r0; k.cp = h_pt[r1] - h_pt[r0];
    r0 = r1;
    if (k.cp == 0) continue;
    SDP_TRY(chunk_begin(c, k));
    SDP_TRY(chunk_sizes(c, k));
    for (int att = 0; att < 3 && k.nsub > 0; att++) SDP_TRY(attempt(c, k, att));
    diag_build_stat(c, k);
    if (k.onePass) SDP_TRY(read_rc(c, k));                                 // (entries as emitted last, re-built reads included)
    c.totalEntries += k.totE;
    SDP_TRY(trace_chains(c, k));
    LRA_HIP_CHECK(ctx, hipGetLastError());
  }
  out->n_subproblem_entries = c.totalEntries;
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(c.st));
  LRA_HIP_CHECK(ctx, hipGetLastError());
  return LRA_OK;
}

}  // namespace

extern "C" int lra_sparse_dp_batch(lra_ctx* ctx, int n_reads, const uint64_t* d_cluster_off, const uint64_t* d_c_start, const uint32_t* d_c_count,
                                   const int32_t* d_c_strand, const uint32_t* d_q, const uint32_t* d_t, const int32_t* d_len,
                                   const uint64_t* d_read_off, const float* d_rate, const lra_sdp_opts* opts, lra_chain_result* out) {
  if (opts && opts->mode != LRA_SDP_CLUSTERS && opts->mode != LRA_SDP_SINGLE_CLUSTER) return lra_set_err(ctx, LRA_ERR_INVALID, "mode must be 0 or 1");
  return sdp_run(ctx, n_reads, d_cluster_off, d_c_start, d_c_count, d_c_strand, d_q, d_t, d_len, d_read_off, d_rate, opts, out, nullptr, nullptr, nullptr);
}

extern "C" int lra_sparse_dp_boxes_batch(lra_ctx* ctx, int n_reads, const uint64_t* d_box_off, const uint32_t* d_qs, const uint32_t* d_qe,
                                         const uint32_t* d_ts, const uint32_t* d_te, const int32_t* d_strand, const int32_t* d_val,
                                         const int32_t* d_num_anchors, const uint64_t* d_read_off, const float* d_rate, const lra_sdp_opts* opts,
                                         lra_chain_result* out) {
  if (!opts || !d_qe || !d_te) return LRA_ERR_INVALID;
  lra_sdp_opts o = *opts;
  o.mode = LRA_SDP_CLUSTERS;                                             // chain decision of the box mode is selected by d_qe
  return sdp_run(ctx, n_reads, d_box_off, nullptr, nullptr, d_strand, d_qs, d_ts, d_val, d_read_off, d_rate, &o, out, d_qe, d_te, d_num_anchors);
}

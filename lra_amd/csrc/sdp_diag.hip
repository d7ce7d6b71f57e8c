// lra_amd/csrc/sdp_diag.hip -- the sparse DP's analysis hooks (sdp.h lists the files): what the driver (sdp.hip) calls between its production steps when one of
// LRA_SDP_DUMP, LRA_SDP_RATIOS, LRA_SDP_STAT, LRA_SDP_DBG, LRA_SDP_BUILD_STAT is set.  Host code only; none of it runs otherwise.
#include "sdp.h"
#include <algorithm>
#include <cstdlib>
#include <string>

namespace lra_sdp {

bool diag_dbg() { static const bool dbg = getenv("LRA_SDP_DBG") != nullptr; return dbg; }
int diag_stat_level() { static const int statEnv = getenv("LRA_SDP_STAT") ? atoi(getenv("LRA_SDP_STAT")) : 0; return statEnv; }
bool diag_build_stat() { static const bool buildStat = getenv("LRA_SDP_BUILD_STAT") != nullptr; return buildStat; }

int diag_dump(const Call& c) {
  const char* dumpPath = getenv("LRA_SDP_DUMP");
  if (!dumpPath) return LRA_OK;
  lra_ctx* ctx = c.ctx; const int n_reads = c.n_reads; const std::vector<uint64_t>& h_frag = c.h_frag;
  static int callNo = 0;
  const int topK = getenv("LRA_SDP_DUMP_TOP") ? atoi(getenv("LRA_SDP_DUMP_TOP")) : 8;
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(c.st));
  std::vector<uint32_t> idx(n_reads);
  for (int i = 0; i < n_reads; i++) idx[i] = (uint32_t)i;
  std::partial_sort(idx.begin(), idx.begin() + std::min(topK, n_reads), idx.end(), [&](uint32_t x, uint32_t y) { return h_frag[x + 1] - h_frag[x] > h_frag[y + 1] - h_frag[y]; });
  std::string pth = std::string(dumpPath) + ".call" + std::to_string(callNo) + (ctx->sdp_inner ? "i" : "") + ".bin";
  if (FILE* f = fopen(pth.c_str(), "wb")) {
    for (int k = 0; k < std::min(topK, n_reads); k++) {
      const uint32_t r = idx[k];
      const uint64_t a0 = h_frag[r], n = h_frag[r + 1] - a0;
      if (n == 0) continue;
      std::vector<uint32_t> q(n), t(n), cl(n); std::vector<int32_t> ln(n); std::vector<uint8_t> sd(n);
      (void)hipMemcpy(q.data(), c.fq + a0, n * 4, hipMemcpyDeviceToHost); (void)hipMemcpy(t.data(), c.ft + a0, n * 4, hipMemcpyDeviceToHost);
      (void)hipMemcpy(ln.data(), c.flen + a0, n * 4, hipMemcpyDeviceToHost); (void)hipMemcpy(cl.data(), c.fcl + a0, n * 4, hipMemcpyDeviceToHost);
      (void)hipMemcpy(sd.data(), c.fstrand + a0, n, hipMemcpyDeviceToHost);
      std::vector<int32_t> coff; std::vector<uint8_t> cst;
      for (uint64_t i = 0; i < n; i++) if (i == 0 || cl[i] != cl[i - 1]) { coff.push_back((int32_t)i); cst.push_back(sd[i]); }
      coff.push_back((int32_t)n);
      int hdr[4] = {c.opts->mode, (int)cst.size(), (int)n, 30000};
      float rate = c.opts->rate;
      fwrite(hdr, 4, 4, f); fwrite(&rate, 4, 1, f); fwrite(coff.data(), 4, coff.size(), f); fwrite(cst.data(), 1, cst.size(), f);
      fwrite(q.data(), 4, n, f); fwrite(t.data(), 4, n, f); fwrite(ln.data(), 4, n, f);
    }
    fclose(f);
  }
  pth = std::string(dumpPath) + ".call" + std::to_string(callNo) + (ctx->sdp_inner ? "i" : "") + ".sizes";
  if (FILE* f = fopen(pth.c_str(), "wb")) { fwrite(c.h_pt.data(), 8, c.n1, f); fclose(f); }
  callNo++;
  return LRA_OK;
}

void diag_ratios(const Call& c, const Chunk& k) {
  if (!getenv("LRA_SDP_RATIOS")) return;
  const int nr = k.nr, r0 = k.r0; const std::vector<uint64_t>& h_pt = c.h_pt;
  std::vector<uint32_t> hE(nr), hN(nr), hD(nr);
  (void)hipMemcpy(hE.data(), k.cntE, (size_t)nr * 4, hipMemcpyDeviceToHost); (void)hipMemcpy(hN.data(), k.cntN, (size_t)nr * 4, hipMemcpyDeviceToHost); (void)hipMemcpy(hD.data(), k.cntD, (size_t)nr * 4, hipMemcpyDeviceToHost);
  std::vector<double> rE, rN, rD; double sE = 0, sP = 0;
  for (int i = 0; i < nr; i++) { const double P = (double)(h_pt[r0 + i + 1] - h_pt[r0 + i]); if (P < 64) continue; rE.push_back(hE[i] / P); rN.push_back(hN[i] / P); rD.push_back(hD[i] / (double)std::max(1u, hE[i])); sE += hE[i]; sP += P; }
  auto pr = [&](const char* nm, std::vector<double>& v) { if (v.empty()) return; std::sort(v.begin(), v.end()); fprintf(stderr, "[sdp ratios] %s: min %.2f p50 %.2f p90 %.2f p99 %.2f p99.9 %.2f max %.2f\n", nm, v[0], v[v.size() / 2], v[v.size() * 9 / 10], v[v.size() * 99 / 100], v[(size_t)(v.size() * 0.999)], v.back()); };
  fprintf(stderr, "[sdp ratios] mode %d inner %d reads %d: entries per point overall %.2f\n", c.opts->mode, (int)c.ctx->sdp_inner, nr, sE / std::max(1.0, sP));
  pr("entries / point", rE); pr("nodes / point", rN); pr("D entries / entries", rD);
}

void diag_stat(const Call& c, const Attempt& a, int n, StatBuf& s) {
  if (!s.d) return;
  unsigned long long hs[40];
  (void)hipStreamSynchronize(c.st); (void)hipMemcpy(hs, s.d, sizeof hs, hipMemcpyDeviceToHost); s.release();
  const double ne = (double)std::max<unsigned long long>(hs[10], 1), ns = (double)std::max<unsigned long long>(hs[11], 1);
  fprintf(stderr, "[sdp-stat] mode %d inner %d reads %d: end points %llu (switch %.2f, %.1f lanes) cycles: switch %.0f deposit %.0f sync %.0f | start points %llu (switch %.2f, %.1f lanes) cycles: switch %.0f "
          "first %.0f small %.0f coop %.0f flush+search %.0f result %.0f sync %.0f | per start point: small iters (max lane) %.2f pops %.2f with-small %.2f coop owners %.3f flush %.2f search rounds %.2f | answer's entry read %.2f, a lane searches %.2f (its Block list changed in the visit %.2f, longest list %.1f), a lane with two candidates or more %.2f\n",
          c.opts->mode, (int)c.ctx->sdp_inner, n, hs[10], hs[12] / ne, hs[14] / ne, hs[0] / ne, hs[2] / ne, hs[8] / ne, hs[11], hs[13] / ns, hs[15] / ns, hs[1] / ns, hs[3] / ns, hs[4] / ns, hs[5] / ns,
          hs[6] / ns, hs[7] / ns, hs[9] / ns, hs[16] / ns, hs[17] / ns, hs[18] / ns, hs[19] / ns, hs[20] / ns, hs[21] / ns, hs[22] / ns, hs[23] / ns, hs[24] / ns, hs[25] / std::max(1.0, (double)hs[23]), hs[26] / ns);
  (void)a;
}

void diag_dbg_begin(const Call& c, Attempt& a) {
  if (!a.dbg) return;
  (void)hipEventCreate(&a.e0); (void)hipEventCreate(&a.e1); (void)hipEventRecord(a.e0, c.st);
}

void diag_dbg_end(const Call& c, const Chunk& k, Attempt& a) {
  if (!a.dbg) return;
  const int nr = k.nr, r0 = k.r0; const std::vector<uint64_t>& h_pt = c.h_pt;
  (void)hipEventRecord(a.e1, c.st); (void)hipEventSynchronize(a.e1);
  float ms = 0; (void)hipEventElapsedTime(&ms, a.e0, a.e1);
  uint64_t mx = 0, tot = 0;
  for (int i = 0; i < nr; i++) { const uint64_t p = h_pt[r0 + i + 1] - h_pt[r0 + i]; mx = std::max(mx, p); tot += p; }
  fprintf(stderr, "[sdp] mode %d inner %d att %d reads %d (of %d) points total %llu max %llu  process %.1f ms\n", c.opts->mode, (int)c.ctx->sdp_inner, a.att, k.nsub, nr,
          (unsigned long long)tot, (unsigned long long)mx, ms);
  (void)hipEventDestroy(a.e0); (void)hipEventDestroy(a.e1);
  if (a.dbgBase && a.nbig > 0) {                                         // the largest read's waves: cycles in each slot and waiting at end points
    std::vector<unsigned long long> tw(256);
    const uint64_t o8 = (a.dbgOff0 + 7) & ~(uint64_t)7;
    (void)hipMemcpy(tw.data(), a.dbgBase + o8, 256 * 8, hipMemcpyDeviceToHost);
    fprintf(stderr, "[sdp]   per wave, M cycles: all | waiting  switch  deposits  publish | queries: set-up  maximization (choose, to-compare, compare+win)  flush+search  result | scan rounds  events | polls  not ready at the first\n");
    for (int w = 0; w < 16; w++) {
      const unsigned long long* o = tw.data() + 16 * w;
      fprintf(stderr, "[sdp]   wave %2d: %6.1f | %6.1f %6.1f %6.1f %6.1f | %6.1f %6.1f (%5.1f %5.1f %5.1f) %6.1f %6.1f | %6llu %6llu | %6llu %6llu\n", w, o[0] * 1e-6, o[1] * 1e-6, o[2] * 1e-6, o[3] * 1e-6, o[4] * 1e-6,
              o[5] * 1e-6, o[6] * 1e-6, o[9] * 1e-6, o[10] * 1e-6, o[11] * 1e-6, o[7] * 1e-6, o[8] * 1e-6, o[12] >> 32, o[12] & 0xffffffffULL, o[13] >> 32, o[13] & 0xffffffffULL);
    }
  }
}

void diag_build_stat(const Call& c, Chunk& k) {
  if (!k.buildStat.d) return;
  unsigned long long hb[16];
  (void)hipStreamSynchronize(c.st); (void)hipMemcpy(hb, k.buildStat.d, sizeof hb, hipMemcpyDeviceToHost); k.buildStat.release(); k.ba.stat = nullptr;
  const double pts = (double)std::max<unsigned long long>(hb[8], 1);
  fprintf(stderr, "[sdp-build-stat] mode %d inner %d reads %d; the wave-per-read builds of 513 .. 16383 points, %llu points; cycles per point: set-up %.1f family %.1f | per level pass A %.1f C %.1f D %.1f E %.1f F %.1f G %.1f\n", c.opts->mode, (int)c.ctx->sdp_inner, k.nr,
          hb[8], hb[0] / pts, hb[7] / pts, hb[1] / pts, hb[2] / pts, hb[3] / pts, hb[4] / pts, hb[5] / pts, hb[6] / pts);
}

}  // namespace lra_sdp

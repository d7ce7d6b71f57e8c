// lra_amd/csrc/map_output.hip -- from a finished batch (lra_map_result) to its records: the per-read tail SetFromSegAlignment / AlignmentsOrder::Update /
// SimpleMapQV / OUTPUT (Map_lowacc.h:600-618, Map_highacc.h:733-789) of both drivers (gfx950 only).  The host pool, the packed record buffer (lra_map_pack,
// lra_map_unpack_host, lra_map_snapshot), the record text on the host (lra_map_records*), the SV signatures (lra_map_svsig*) and the piece table of the
// device records (lra_map_records_device*).  Nothing here maps a read.
#include "common.h"
#include "seed_state.h"
#include "map_state.h"
#include "records.h"
#include "emit_fmt.h"
#include "emit_bam.h"
#include <chrono>
#include <math.h>
#include <stdlib.h>
#include <algorithm>
#include <thread>
#include <mutex>

// ---------------------------------------------------------------------------------------------------------------- records (host)
// lra_map_snapshot copies what the records need from the context's result buffers to the host (so the next batch may overwrite them);
// lra_map_records_host turns a snapshot into text with host threads only -- it touches neither the context nor the device, so it runs
// beside the next batch's lra_map_reads_lowacc_batch.  lra_map_records = both, with the reference's two-call output convention.
struct lra_map_host {
  int32_t n_reads = 0, num_aln = 1; uint64_t nJ = 0, nA = 0;
  std::vector<uint64_t> jo, roff, boff; std::vector<int32_t> strand, supp, sec, n0, n1, chrom, counts, blocks; std::vector<float> fval;
  lra_pod_buf<uint32_t> runs;                              // the CIGAR runs: 0.7 GB per 32768 reads of 30 kb
  std::vector<uint32_t> rstat, ends;                       // ends: per alignment first block's qPos, last block's qPos + length
  std::vector<uint8_t> reached;
  std::vector<uint64_t> chrom_pos;
  std::vector<std::string> segText; std::vector<uint32_t> segStart;   // print format 'a' only
  bool has_md = false; std::vector<uint64_t> md_off; std::string md;  // LRA_PACK_MD: alignment a's MD:Z value is md[md_off[a], md_off[a + 1])
  bool has_sv = false; std::vector<uint64_t> sv_off; std::vector<lra_svsig_rec> sv_rec; std::string sv_seq;   // LRA_PACK_SVSIG: alignment a's signatures are sv_rec[sv_off[a], sv_off[a + 1])
  lra_text_buf sv_text; std::vector<uint64_t> sv_rec_off;  // what lra_map_svsig_host produced last
  lra_text_buf text; std::vector<uint64_t> rec_off;        // what lra_map_records_host produced last
};

namespace {
template <typename T>
int fetch(lra_ctx* ctx, std::vector<T>& v, const T* d, size_t n) {
  v.resize(n);
  if (n && d) LRA_HIP_CHECK(ctx, hipMemcpy(v.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
  return LRA_OK;
}
__global__ void k_block_ends(uint64_t nA, const uint64_t* __restrict__ boff, const int32_t* __restrict__ blocks, uint32_t* __restrict__ ends) {
  const uint64_t a = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= nA) return;
  const uint64_t b0 = boff[a], b1 = boff[a + 1];
  ends[2 * a] = b1 > b0 ? (uint32_t)blocks[3 * b0] : 0;
  ends[2 * a + 1] = b1 > b0 ? (uint32_t)(blocks[3 * (b1 - 1)] + blocks[3 * (b1 - 1) + 2]) : 0;
}
// LRA_PACK_MD / LRA_PACK_SVSIG: alignment a's read strand and chromosome in the result's own arrays (k_aln_address's offsets, from the read offsets the strands carry)
__global__ void k_md_address(uint64_t nA, const uint32_t* __restrict__ aln_read, const int32_t* __restrict__ strand, const int32_t* __restrict__ chrom,
                             const uint64_t* __restrict__ read_off, uint64_t rc_base, const uint64_t* __restrict__ chrom_pos, uint64_t* __restrict__ q_off,
                             uint64_t* __restrict__ t_off) {
  const uint64_t a = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= nA) return;
  q_off[a] = read_off[aln_read[a]] + (strand[a] ? rc_base : 0);
  t_off[a] = chrom_pos[chrom[a]];
}
// lra_map_records_device with LRA_PACK_SVSIG: no alignment of a read with a non-zero status word (flagged or handed back) prints a signature
__global__ void k_sv_skip(uint64_t nA, int n_reads, const uint32_t* __restrict__ aln_read, const uint32_t* __restrict__ read_status, uint8_t* __restrict__ skip) {
  const uint64_t a = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= nA) return;
  const uint32_t r = aln_read[a];
  skip[a] = r < (uint32_t)n_reads && read_status[r] ? 1 : 0;
}
// ... and read r's lines are those of alignments job_aln_off[r * num_aln] .. job_aln_off[(r + 1) * num_aln)
__global__ void k_sv_rec_off(int n_reads, int num_aln, uint64_t nJ, uint64_t nA, const uint64_t* __restrict__ job_aln_off, const uint64_t* __restrict__ aln_off,
                             uint64_t* __restrict__ rec_off) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r > n_reads) return;
  const uint64_t j = min((uint64_t)r * num_aln, nJ);
  rec_off[r] = aln_off[min(job_aln_off[j], nA)];
}
}  // namespace

extern "C" void lra_map_host_free(lra_map_host* h) { delete h; }
extern "C" uint64_t lra_map_host_flagged(const lra_map_host* h, const uint32_t** status) {
  if (status) *status = nullptr;
  if (!h) return 0;
  uint64_t n = 0;
  for (uint32_t v : h->rstat) n += v != 0 && v != (uint32_t)LRA_ST_DEFERRED;   // (a handed-back read is not a flagged one)
  if (status && !h->rstat.empty()) *status = h->rstat.data();
  return n;
}

namespace {
std::mutex g_pool_mu;
struct PoolBlock { void* p; size_t cap; };
std::vector<PoolBlock> g_pool;                                           // at most POOL_KEEP blocks, the largest ones
constexpr size_t POOL_KEEP = 6, POOL_MIN = 8u << 20;
}  // namespace
// the record threads' parts of a batch's text (lra_map_records_host): strings kept between batches with their capacity -- a part is ~100 MB, and a fresh one is
// 25 000 page faults and a chain of doubling reallocations
namespace {
std::mutex g_parts_mu;
std::vector<std::string> g_parts;
size_t g_parts_bytes = 0;                                                // capacity held by the pool
size_t parts_cap() {                                                     // at most this much is kept between batches (LRA_PARTS_POOL_MB; lra_map_host_trim lowers what is held now)
  static const size_t cap = [] { const char* e = getenv("LRA_PARTS_POOL_MB"); return (size_t)(e ? std::max(0, atoi(e)) : 4096) << 20; }();
  return cap;
}
std::string part_take(size_t want) {
  std::string s;
  {
    std::lock_guard<std::mutex> lk(g_parts_mu);
    int best = -1;                                                       // the smallest string that holds `want`, else the largest there is
    for (int i = 0; i < (int)g_parts.size(); i++) {
      const size_t c = g_parts[i].capacity();
      if (best < 0) { best = i; continue; }
      const size_t b = g_parts[best].capacity();
      if (b >= want ? (c >= want && c < b) : c > b) best = i;
    }
    if (best >= 0) { g_parts_bytes -= g_parts[best].capacity(); s.swap(g_parts[best]); g_parts.erase(g_parts.begin() + best); }
  }
  s.clear();
  if (s.capacity() < want) s.reserve(want);
  return s;
}
void part_give(std::string& s) {
  s.clear();
  std::lock_guard<std::mutex> lk(g_parts_mu);
  if (g_parts.size() < 64 && s.capacity() >= (8u << 20) && g_parts_bytes + s.capacity() <= parts_cap()) { g_parts_bytes += s.capacity(); g_parts.emplace_back(); g_parts.back().swap(s); }
  else std::string().swap(s);
}
}  // namespace
// Host memory the record stage keeps between batches (the threads' text parts): released down to keep_bytes (0: all of it).  Returns the bytes still held.
extern "C" uint64_t lra_map_host_trim(uint64_t keep_bytes) {
  std::lock_guard<std::mutex> lk(g_parts_mu);
  while (!g_parts.empty() && g_parts_bytes > keep_bytes) {
    int big = 0;
    for (int i = 1; i < (int)g_parts.size(); i++) if (g_parts[i].capacity() > g_parts[big].capacity()) big = i;
    g_parts_bytes -= g_parts[big].capacity();
    g_parts.erase(g_parts.begin() + big);
  }
  if (g_parts.empty()) std::vector<std::string>().swap(g_parts);
  return g_parts_bytes;
}
void* lra_host_pool_get(size_t bytes, size_t* cap) {
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    int best = -1;
    for (int i = 0; i < (int)g_pool.size(); i++) if (g_pool[i].cap >= bytes && (best < 0 || g_pool[i].cap < g_pool[best].cap)) best = i;
    if (best >= 0 && g_pool[best].cap <= 2 * bytes + POOL_MIN) { void* p = g_pool[best].p; *cap = g_pool[best].cap; g_pool.erase(g_pool.begin() + best); return p; }
  }
  *cap = bytes;
  return malloc(bytes);
}
void lra_host_pool_put(void* p, size_t cap) {
  if (!p) return;
  if (cap >= POOL_MIN) {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    if (g_pool.size() < POOL_KEEP) { g_pool.push_back({p, cap}); return; }
    int smallest = 0;
    for (int i = 1; i < (int)g_pool.size(); i++) if (g_pool[i].cap < g_pool[smallest].cap) smallest = i;
    if (g_pool[smallest].cap < cap) { void* q = g_pool[smallest].p; g_pool[smallest] = {p, cap}; p = q; }
  }
  free(p);
}

// ---- the record buffer of a batch: everything the host tail needs, packed into one device buffer (what a rank sends to rank 0)
//   int64 header[16] = {magic, n_reads, num_aln, nJ, nA, n_blocks (0 unless with_blocks), n_runs, n_chrom, has_reached, has_rstat, ...}
//   then, each padded to 8 bytes:  chrom_pos u64[n_chrom+1] | reached u8[nJ] | rstat u32[n_reads] | jo u64[nJ+1] | strand, supp, sec, n0, n1, chrom
//   i32[nA] each | fval f32[nA] | counts i32[18 nA] | boff u64[nA+1] | ends u32[2 nA] | roff u64[nA+1] | runs u32[n_runs] | blocks i32[3 n_blocks]
//   | (LRA_PACK_MD: header[10] = MD bytes, header[11] = 1) md_off u64[nA+1] | md u8[header[10]]
//   | (LRA_PACK_SVSIG: header[12] = the section's bytes, header[13] = 1) sig_off u64[nA+1] | lra_svsig_rec[sig_off[nA]] | the sequences u8[]
namespace {
constexpr int64_t PACK_MAGIC = 0x4c52414d41503031LL;   // "LRAMAP01"
inline size_t pad8(size_t n) { return (n + 7) & ~(size_t)7; }
struct PackLayout {
  size_t off[17]; size_t total;
  PackLayout(uint64_t n_reads, uint64_t nJ, uint64_t nA, uint64_t n_blocks, uint64_t n_runs, uint64_t n_chrom, bool md = false, uint64_t md_bytes = 0,
             uint64_t sv_bytes = 0) {
    const size_t sz[17] = {16 * 8, (n_chrom + 1) * 8, nJ, n_reads * 4, (nJ + 1) * 8, nA * 4, nA * 4, nA * 4, nA * 4, nA * 4, nA * 4, nA * 4, 18 * nA * 4, (nA + 1) * 8,
                           2 * nA * 4, (nA + 1) * 8, n_runs * 4};
    size_t at = 0;
    for (int i = 0; i < 17; i++) { off[i] = at; at += pad8(sz[i]); }
    blocks_off = at; at += pad8(3 * n_blocks * 4);
    md_off = at; if (md) at += pad8((nA + 1) * 8);
    md_text = at; if (md) at += pad8(md_bytes);
    sv_off = at; at += sv_bytes;
    total = at;
  }
  size_t blocks_off, md_off, md_text, sv_off;
};
// the SV section: sig_off, the records, the sequences
inline size_t sv_section_bytes(uint64_t nA, uint64_t n_sig, uint64_t n_seq) { return (nA + 1) * 8 + n_sig * sizeof(lra_svsig_rec) + pad8(n_seq); }
static_assert(sizeof(lra_svsig_rec) == 24, "lra_svsig_rec is part of the pack's layout");
}  // namespace

extern "C" int lra_map_pack(lra_ctx* ctx, const lra_map_result* res, int with_blocks, const void** d_buf, uint64_t* bytes) {
  if (!ctx || !res || !d_buf || !bytes) return LRA_ERR_INVALID;
  lra_map_state* m = ctx->map;
  if (!m) return LRA_ERR_INVALID;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (with_blocks & ~(LRA_PACK_BLOCKS | LRA_PACK_MD | LRA_PACK_SVSIG | LRA_PACK_NORUNS)) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_map_pack: unknown flags 0x%x", with_blocks);
  const bool withMd = (with_blocks & LRA_PACK_MD) != 0, withSv = (with_blocks & LRA_PACK_SVSIG) != 0;
  const uint64_t nR = (uint64_t)res->n_reads, nJ = res->n_jobs, nA = res->n_alignments, nB = (with_blocks & LRA_PACK_BLOCKS) ? res->n_blocks : 0,
                 nRuns = (with_blocks & LRA_PACK_NORUNS) ? 0 : res->n_runs;           // LRA_PACK_NORUNS: the device record stage reads the runs where they are
  const uint64_t nCh = m->chrom_pos.size() - 1;
  // opts.printMD, opts.Printsvsig: the MD strings / SV signatures of the result's final blocks, from the reads on their strands (res->d_strands, addressed by the
  // read offsets behind them) and the genome
  lra_md_result md; memset(&md, 0, sizeof md);
  lra_svsig_result sv; memset(&sv, 0, sizeof sv);
  if ((withMd || withSv) && nA) {
    if (!res->d_strands || !res->d_aln_read || !res->d_strand || !res->d_chrom || !res->d_blocks || !res->d_block_off)
      return lra_set_err(ctx, LRA_ERR_INVALID, "LRA_PACK_MD / LRA_PACK_SVSIG: the result has no reads / blocks to work on");
    if (!ctx->seed || !ctx->seed->genome || !m->d_chrom_pos) return lra_set_err(ctx, LRA_ERR_INVALID, "LRA_PACK_MD / LRA_PACK_SVSIG: genome not loaded");
    uint64_t* adr = (uint64_t*)lra_ensure(ctx, 187, 2 * (nA + 1) * 8);
    if (!adr) return LRA_ERR_NOMEM;
    const uint64_t* ro = (const uint64_t*)(res->d_strands + lra_strands_ro_at(res->rc_base));
    hipLaunchKernelGGL(k_md_address, dim3((unsigned)((nA + 255) / 256)), dim3(256), 0, st, nA, res->d_aln_read, res->d_strand, res->d_chrom, ro, res->rc_base,
                       (const uint64_t*)m->d_chrom_pos, adr, adr + nA + 1);
    int rcm = LRA_OK;
    if (withMd) rcm = lra_md_strings_batch(ctx, (int)nA, res->d_blocks, res->d_block_off, res->d_strands, adr, nullptr, (const char*)ctx->seed->genome, adr + nA + 1, &md);
    if (!rcm && withSv)
      rcm = lra_sv_signatures_batch(ctx, (int)nA, res->d_blocks, res->d_block_off, res->d_strands, adr, nullptr, (const char*)ctx->seed->genome, adr + nA + 1,
                                    ctx->svsig_len, &sv);
    if (rcm) return rcm;
  }
  const uint64_t svBytes = withSv ? sv_section_bytes(nA, sv.n_sig, sv.n_seq_bytes) : 0;
  const PackLayout L(nR, nJ, nA, nB, nRuns, nCh, withMd, md.n_bytes, svBytes);
  char* buf = (char*)lra_ensure(ctx, 84, L.total + 64);
  if (!buf) return LRA_ERR_NOMEM;
  const int64_t hdr[16] = {PACK_MAGIC, (int64_t)nR, std::max(res->num_aln, 1), (int64_t)nJ, (int64_t)nA, (int64_t)nB, (int64_t)nRuns, (int64_t)nCh,
                           res->d_job_reached ? 1 : 0, res->d_read_status ? 1 : 0, (int64_t)md.n_bytes, withMd ? 1 : 0, (int64_t)svBytes, withSv ? 1 : 0, 0, 0};
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(buf + L.off[0], hdr, sizeof hdr, hipMemcpyHostToDevice, st));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(buf + L.off[1], m->d_chrom_pos, (nCh + 1) * 8, hipMemcpyDeviceToDevice, st));
  auto put = [&](int slot, const void* src, size_t n) -> hipError_t { return (n && src) ? hipMemcpyAsync(buf + L.off[slot], src, n, hipMemcpyDeviceToDevice, st) : hipSuccess; };
  if (nA) {
    uint32_t* d_ends = (uint32_t*)(buf + L.off[14]);
    hipLaunchKernelGGL(k_block_ends, dim3((unsigned)((nA + 255) / 256)), dim3(256), 0, st, nA, res->d_block_off, res->d_blocks, d_ends);
  }
  LRA_HIP_CHECK(ctx, put(2, res->d_job_reached, nJ));
  LRA_HIP_CHECK(ctx, put(3, res->d_read_status, nR * 4));
  LRA_HIP_CHECK(ctx, put(4, res->d_job_aln_off, nJ ? (nJ + 1) * 8 : 0));
  LRA_HIP_CHECK(ctx, put(5, res->d_strand, nA * 4)); LRA_HIP_CHECK(ctx, put(6, res->d_supp, nA * 4)); LRA_HIP_CHECK(ctx, put(7, res->d_secondary, nA * 4));
  LRA_HIP_CHECK(ctx, put(8, res->d_n0, nA * 4)); LRA_HIP_CHECK(ctx, put(9, res->d_n1, nA * 4)); LRA_HIP_CHECK(ctx, put(10, res->d_chrom, nA * 4));
  LRA_HIP_CHECK(ctx, put(11, res->d_first_sdp_value, nA * 4)); LRA_HIP_CHECK(ctx, put(12, res->d_counts, 18 * nA * 4));
  LRA_HIP_CHECK(ctx, put(13, res->d_block_off, nA ? (nA + 1) * 8 : 0)); LRA_HIP_CHECK(ctx, put(15, res->d_run_off, nA ? (nA + 1) * 8 : 0));
  LRA_HIP_CHECK(ctx, put(16, res->d_runs, nRuns * 4));
  if (nB) LRA_HIP_CHECK(ctx, hipMemcpyAsync(buf + L.blocks_off, res->d_blocks, 3 * nB * 4, hipMemcpyDeviceToDevice, st));
  if (withMd) {
    if (nA) LRA_HIP_CHECK(ctx, hipMemcpyAsync(buf + L.md_off, md.d_md_off, (nA + 1) * 8, hipMemcpyDeviceToDevice, st));
    else LRA_HIP_CHECK(ctx, hipMemsetAsync(buf + L.md_off, 0, 8, st));
    if (md.n_bytes) LRA_HIP_CHECK(ctx, hipMemcpyAsync(buf + L.md_text, md.d_md, md.n_bytes, hipMemcpyDeviceToDevice, st));
  }
  if (withSv) {
    char* w = buf + L.sv_off;
    if (nA) LRA_HIP_CHECK(ctx, hipMemcpyAsync(w, sv.d_sig_off, (nA + 1) * 8, hipMemcpyDeviceToDevice, st));
    else LRA_HIP_CHECK(ctx, hipMemsetAsync(w, 0, 8, st));
    w += (nA + 1) * 8;
    if (sv.n_sig) LRA_HIP_CHECK(ctx, hipMemcpyAsync(w, sv.d_sig, sv.n_sig * sizeof(lra_svsig_rec), hipMemcpyDeviceToDevice, st));
    w += sv.n_sig * sizeof(lra_svsig_rec);
    if (sv.n_seq_bytes) {
      LRA_HIP_CHECK(ctx, hipMemsetAsync(w + (pad8(sv.n_seq_bytes) - 8), 0, 8, st));                     // (the padding is part of the pack)
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(w, sv.d_seq, sv.n_seq_bytes, hipMemcpyDeviceToDevice, st));
    }
  }
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  *d_buf = buf; *bytes = L.total;
  return LRA_OK;
}

// a packed record buffer (host memory) -> snapshot
extern "C" int lra_map_unpack_host(const void* h_buf, uint64_t bytes, lra_map_host** out) {
  if (!h_buf || !out || bytes < 16 * 8) return LRA_ERR_INVALID;
  *out = nullptr;
  const char* b = (const char*)h_buf;
  int64_t hdr[16];
  memcpy(hdr, b, sizeof hdr);
  if (hdr[0] != PACK_MAGIC) return LRA_ERR_INVALID;
  const uint64_t nR = (uint64_t)hdr[1], nJ = (uint64_t)hdr[3], nA = (uint64_t)hdr[4], nB = (uint64_t)hdr[5], nRuns = (uint64_t)hdr[6], nCh = (uint64_t)hdr[7];
  const bool hasMd = hdr[10] != 0 || hdr[11] != 0;                      // (packs written before LRA_PACK_MD have zeros there)
  if (hdr[10] < 0) return LRA_ERR_INVALID;
  const bool hasSv = hdr[12] != 0 || hdr[13] != 0;                      // (packs written before LRA_PACK_SVSIG have zeros there)
  if (hasSv && (hdr[12] < (int64_t)((nA + 1) * 8) || (hdr[12] & 7))) return LRA_ERR_INVALID;
  const PackLayout L(nR, nJ, nA, nB, nRuns, nCh, hasMd, (uint64_t)hdr[10], hasSv ? (uint64_t)hdr[12] : 0);
  if (L.total > bytes) return LRA_ERR_INVALID;
  lra_map_host* h = new lra_map_host();
  h->n_reads = (int32_t)nR; h->num_aln = (int)hdr[2]; h->nJ = nJ; h->nA = nA;
  auto get = [&](auto& v, int slot, size_t n) { v.resize(n); if (n) memcpy(v.data(), b + L.off[slot], n * sizeof(v[0])); };
  get(h->chrom_pos, 1, nCh + 1);
  if (hdr[8]) get(h->reached, 2, nJ);
  if (hdr[9]) get(h->rstat, 3, nR);
  get(h->jo, 4, nJ ? nJ + 1 : 0);
  get(h->strand, 5, nA); get(h->supp, 6, nA); get(h->sec, 7, nA); get(h->n0, 8, nA); get(h->n1, 9, nA); get(h->chrom, 10, nA); get(h->fval, 11, nA);
  get(h->counts, 12, 18 * nA); get(h->boff, 13, nA ? nA + 1 : 0); get(h->ends, 14, 2 * nA); get(h->roff, 15, nA ? nA + 1 : 0);
  if (nRuns) {                                                           // the one large array: uninitialised (pooled) memory, copied by a few threads
    if (!h->runs.alloc(nRuns)) { delete h; return LRA_ERR_NOMEM; }
    const char* src = b + L.off[16]; char* dst = (char*)h->runs.data(); const size_t tot = nRuns * 4;
    const int T = tot > (64u << 20) ? std::min(16, lra_host_threads()) : 1;
    auto cp = [&](int t) { const size_t lo = tot * t / T, hi = tot * (t + 1) / T; memcpy(dst + lo, src + lo, hi - lo); };
    if (T == 1) cp(0);
    else { std::vector<std::thread> th; for (int t = 0; t < T; t++) th.emplace_back(cp, t); for (auto& x : th) x.join(); }
  }
  if (nB) { h->blocks.resize(3 * nB); memcpy(h->blocks.data(), b + L.blocks_off, 3 * nB * 4); }
  if (hasMd) {
    h->has_md = true;
    h->md_off.resize(nA + 1);
    memcpy(h->md_off.data(), b + L.md_off, (nA + 1) * 8);
    for (uint64_t a = 0; a < nA; a++)
      if (h->md_off[a] > h->md_off[a + 1] || h->md_off[a + 1] > (uint64_t)hdr[10]) { delete h; return LRA_ERR_INVALID; }
    h->md.assign(b + L.md_text, (size_t)hdr[10]);
  }
  if (hasSv) {
    // sig_off runs from 0 without a step back; the records and the sequences fill what the section has behind it (the sequences padded to 8 bytes); every
    // record names a gap of its own alignment and bases inside the sequences
    h->has_sv = true;
    const char* w = b + L.sv_off;
    size_t left = (size_t)hdr[12] - (nA + 1) * 8;
    h->sv_off.resize(nA + 1);
    memcpy(h->sv_off.data(), w, (nA + 1) * 8); w += (nA + 1) * 8;
    bool ok = h->sv_off[0] == 0 && (h->boff.size() == nA + 1 || nA == 0);
    for (uint64_t a = 0; ok && a < nA; a++) ok = h->sv_off[a] <= h->sv_off[a + 1];
    const uint64_t nS = h->sv_off[nA];
    ok = ok && nS <= left / sizeof(lra_svsig_rec);
    if (ok) {
      h->sv_rec.resize(nS);
      if (nS) memcpy(h->sv_rec.data(), w, nS * sizeof(lra_svsig_rec));
      w += nS * sizeof(lra_svsig_rec); left -= nS * sizeof(lra_svsig_rec);
      for (uint64_t a = 0; ok && a < nA; a++) {
        const uint64_t nb = h->boff[a + 1] - h->boff[a];
        for (uint64_t x = h->sv_off[a]; ok && x < h->sv_off[a + 1]; x++) {
          const lra_svsig_rec& r = h->sv_rec[x];
          ok = (r.kind == LRA_SV_INS || r.kind == LRA_SV_DEL) && r.len > 0 && (uint64_t)r.block + 1 < nb && r.seq_off <= left && r.len <= left - r.seq_off;
        }
      }
    }
    if (!ok) { delete h; return LRA_ERR_INVALID; }
    h->sv_seq.assign(w, left);
  }
  *out = h;
  return LRA_OK;
}

extern "C" int lra_map_snapshot(lra_ctx* ctx, const lra_map_result* res, int with_blocks, lra_map_host** out) {
  if (!ctx || !res || !out) return LRA_ERR_INVALID;
  *out = nullptr;
  const void* d_buf = nullptr; uint64_t bytes = 0;
  int rc = lra_map_pack(ctx, res, with_blocks, &d_buf, &bytes);
  if (rc) return rc;
  char* hb = (char*)lra_pinned(ctx, bytes);                                // (page-locked and kept: see lra_pinned)
  if (!hb) return LRA_ERR_NOMEM;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(hb, d_buf, bytes, hipMemcpyDeviceToHost, ctx->stream));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  lra_map_host* h = nullptr;
  if ((rc = lra_map_unpack_host(hb, bytes, &h))) return rc;
  if (with_blocks & LRA_PACK_BLOCKS) {
    // print format 'a': the pairwise text needs the chromosome bases under every alignment (and the read on its strand)
    lra_map_state* m = ctx->map;
    if (!ctx->seed || !ctx->seed->genome) { delete h; return lra_set_err(ctx, LRA_ERR_INVALID, "genome not loaded"); }
    const size_t nA = h->nA;
    h->segText.resize(nA); h->segStart.assign(nA, 0);
    for (size_t a = 0; a < nA; a++) {
      const uint64_t b0 = h->boff[a], b1 = h->boff[a + 1];
      if (b1 == b0) continue;
      const uint32_t t0 = (uint32_t)h->blocks[3 * b0 + 1], t1 = (uint32_t)(h->blocks[3 * (b1 - 1) + 1] + h->blocks[3 * (b1 - 1) + 2]);
      h->segStart[a] = t0;
      h->segText[a].resize((size_t)(t1 - t0) + 1);
      if (hipMemcpy(&h->segText[a][0], ctx->seed->genome + m->chrom_pos[h->chrom[a]] + t0, t1 - t0, hipMemcpyDeviceToHost) != hipSuccess) { delete h; return LRA_ERR_HIP; }
    }
  }
  *out = h;
  return LRA_OK;
}

// ---- lra_map_records_device, the host half: the records as a piece table (records.h) ------------------------------------------------------------
namespace {
// BAM records: seq = the ranges lra_bam_pack_seq_batch packs, as (reverse strand << 63) | (read << 32) | first base until the read offsets are known; qual = the
// requests of lra_bam_phred_batch; rec_first = every record's first piece
struct lra_piece_part {                                                  // a thread's range of reads; first: every read's first piece
  std::vector<lra_rec_piece> pieces; std::string blob; std::vector<uint64_t> first;
  std::vector<lra_bam_seq_range> seq; std::vector<lra_bam_qual_req> qual; std::vector<uint64_t> rec_first;
};
struct lra_piece_table {
  std::vector<lra_rec_piece> pieces; std::string blob; std::vector<uint64_t> read_piece;
  bool bam = false; int cigar_limit = 65535; int bad_read = -1;          // in: BAM records; out: the read whose record could not be written
  std::vector<lra_bam_seq_range> seq; std::vector<lra_bam_qual_req> qual; std::vector<uint64_t> rec_first;
};
// emit_fmt.h's sink: the short fields into the blob (literals that follow each other inside a read are one piece), the long ones as references
struct lra_piece_sink {
  lra_piece_part& P; size_t barrier;                                     // the read's first piece: no literal is joined across it
  const lra_aln_record* base; const uint64_t* aln;                       // the read's records and their alignments
  uint32_t read; int32_t read_len;
  const int32_t* chrom = nullptr; const uint64_t* roff = nullptr; int limit = 65535;   // BAM records: per alignment its chromosome and its runs' offsets
  void push(uint32_t kind, uint64_t n, uint64_t src) { P.pieces.push_back(lra_rec_piece{kind, (uint32_t)n, src}); }
  void lit(const std::string& t) {
    if (t.empty()) return;
    if (P.pieces.size() > barrier && P.pieces.back().kind == LRA_PIECE_LIT && P.pieces.back().src + P.pieces.back().len == P.blob.size() &&
        (uint64_t)P.pieces.back().len + t.size() < 0xffffffffull) P.pieces.back().len += (uint32_t)t.size();
    else push(LRA_PIECE_LIT, t.size(), P.blob.size());
    P.blob += t;
  }
  void cigar(const lra_aln_record& x) { push(LRA_PIECE_CIGAR, 0, aln[&x - base]); }
  void md(const lra_aln_record& x) { push(LRA_PIECE_MD, 0, aln[&x - base]); }
  void pairwise(const lra_aln_record& x) { push(LRA_PIECE_PAIRWISE, 0, aln[&x - base]); }
  void range(uint32_t kind, size_t from, size_t n) {                     // a range of the read, cut to it
    const size_t L = (size_t)std::max(read_len, 0);
    from = std::min(from, L); n = std::min(n, L - from);
    if (n) push(kind, n, ((uint64_t)read << 32) | (uint64_t)from);
  }
  void seq(const lra_aln_record& r, size_t from, size_t n) { range(r.strand ? LRA_PIECE_SEQ_RC : LRA_PIECE_SEQ_FW, from, n); }
  void qual(const lra_aln_record& r) { range(LRA_PIECE_QUAL, 0, (size_t)r.read_len); }   // (an unaligned read's string goes out as it is, a leading '*' too)
  void qual_sub(const lra_aln_record&, size_t pos, size_t n) { range(LRA_PIECE_QUAL, pos, n); }
  // emit_bam.h's part
  void rec_begin() { P.rec_first.push_back(P.pieces.size()); barrier = P.pieces.size(); }
  int32_t ref_id(const lra_aln_record& x) const { return chrom[aln[&x - base]]; }
  uint64_t n_runs(const lra_aln_record& x) const { const uint64_t a = aln[&x - base]; return roff[a + 1] - roff[a]; }
  int cigar_limit() const { return limit; }
  void bam_cigar(const lra_aln_record& x) { push(LRA_PIECE_BAM_CIGAR, 0, aln[&x - base]); }
  void bam_seq(const lra_aln_record& r, size_t from, size_t n) {
    const size_t L = (size_t)std::max(read_len, 0);
    from = std::min(from, L); n = std::min(n, L - from);
    if (!n) return;
    push(LRA_PIECE_BAM_SEQ, 0, P.seq.size());
    P.seq.push_back(lra_bam_seq_range{((uint64_t)(r.strand ? 1 : 0) << 63) | ((uint64_t)read << 32) | (uint64_t)from, (uint64_t)n});
  }
  void bam_qual(const lra_aln_record&, size_t pos, size_t n, bool have) {
    if (!n) return;
    push(LRA_PIECE_BAM_QUAL, 0, P.qual.size());
    P.qual.push_back(lra_bam_qual_req{have ? read : 0xffffffffu, (uint32_t)pos, (uint32_t)n, 0});
  }
};
// lra_output_read_str (rank.hip; OUTPUT, Mapping_ultility.h:453-493) for the three formats the device stage writes
int piece_output_read(const lra_aln_group* groups, const int32_t* index, int n_groups, lra_aln_record* recs, int print_num_aln, char format, int hard_clip,
                      const char* passthrough, const lra_aln_record* unaligned_rec, lra_piece_sink& k) {
  if (n_groups > 0 && groups[index[0]].count > 0) {
    const int na = std::min(n_groups, print_num_aln);
    for (int a = 0; a < na; a++) {
      const lra_aln_group& G = groups[index[a]];
      lra_aln_record* S = recs + G.first;
      for (int s = G.count - 1; s >= 0; s--) {
        S[s].order = G.count - 1 - s;
        const int rc = format == 's' ? lra_fmt_sam(S, G.count, s, hard_clip, passthrough, k) : format == 'B' ? lra_fmt_bam(S, G.count, s, hard_clip, passthrough, k) :
                       format == 'a' ? lra_fmt_pairwise(S[s], k) : lra_fmt_paf(&S[s], 1, k);
        if (rc) return rc;
      }
    }
  } else if (format == 's' && unaligned_rec) return lra_fmt_sam_simple_unaligned(*unaligned_rec, passthrough, k);
  else if (format == 'B' && unaligned_rec) return lra_fmt_bam_unaligned(*unaligned_rec, passthrough, k);
  return LRA_OK;
}
}  // namespace

// passthrough: the text behind every read's records; tags (when not NULL) instead: one per read, NULL = none (--passthrough of SAM / BAM input)
static int records_host(lra_map_host* h, const lra_map_opts* o, const char* const* names, const char* const* reads, const char* const* quals,
                        const int32_t* read_len, const char* const* chrom_names, const char* passthrough, const char* const* tags, int n_threads,
                        const char** text, uint64_t* len, const uint64_t** rec_off, lra_piece_table* PT = nullptr, bool pieceMd = false) {
  if (!h || !o || !names || (!reads && !PT) || !read_len || !chrom_names || !len) return LRA_ERR_INVALID;
  if (PT && o->printFormat != 's' && o->printFormat != 'P' && o->printFormat != 'a') return LRA_ERR_INVALID;
  const size_t nA = h->nA, nJ = h->nJ;
  (void)nA;
  const int na = h->num_aln;
  const std::vector<uint64_t>& jo = h->jo; const std::vector<uint64_t>& roff = h->roff; const std::vector<uint64_t>& boff = h->boff;
  const std::vector<int32_t>&strand = h->strand, &supp = h->supp, &sec = h->sec, &n0 = h->n0, &n1 = h->n1, &chrom = h->chrom, &counts = h->counts, &blocks = h->blocks;
  const std::vector<float>& fval = h->fval; const lra_pod_buf<uint32_t>& runs = h->runs; const std::vector<uint32_t>&rstat = h->rstat, &ends = h->ends; const std::vector<uint8_t>& reached = h->reached;
  const bool pairwise = o->printFormat == 'a' && !PT;                     // (piece mode: the rows are the device's, from the blocks where they are)
  const bool withMd = (PT ? pieceMd : h->has_md) && o->printFormat == 's';   // (only PrintSAM prints MD; SimplePrintSAM, PrintPAF, PrintBed do not)
  if (withMd && !PT && h->md_off.size() != nA + 1) return LRA_ERR_INVALID;
  if (!PT && nA && roff.size() == nA + 1 && runs.size() < roff[nA]) return LRA_ERR_INVALID;   // a snapshot packed with LRA_PACK_NORUNS has no CIGAR to print
  const char pieceFormat = (PT && PT->bam) ? 'B' : (char)o->printFormat;  // ('B': the BAM form of 's', emit_bam.h)
  const bool hi = !o->bypassClustering;                                   // MapRead_highacc's tail (Map_highacc.h:733-789)
  if (pairwise && h->segText.size() != h->nA) return LRA_ERR_INVALID;
  // every read is independent: host threads take contiguous ranges of reads, each builds its own text; ranges are joined in read order
  const int n_reads = h->n_reads;
  int T = n_threads > 0 ? n_threads : lra_host_threads();                  // n_threads = 0: what the host allows (a 30 kb read's record is ~43 KB of text: 1.4 GB per 32768 reads)
  T = std::max(1, std::min(T, n_reads / 32 + 1));
  if (const char* e = getenv("LRA_RECORD_THREADS")) T = std::max(1, atoi(e));
  std::vector<std::string> part(T);
  std::vector<lra_piece_part> ppart(PT ? T : 0);                         // lra_map_records_device: the threads write pieces, not text
  std::vector<std::vector<uint64_t>> plen(T);
  std::vector<int> prc(T, LRA_OK), pbad(T, -1);
  auto work = [&](int tix) {
    const int lo = (int)((long)n_reads * tix / T), hi = (int)((long)n_reads * (tix + 1) / T);
    std::string& text = part[tix];
    if (!PT) {                                                            // room for the range's text: the reads, their CIGAR runs (~3.3 characters each), the tags
      size_t want = 4096;
      for (int r = lo; r < hi; r++) want += (size_t)read_len[r] + 700;
      if (nJ && jo.size() > (size_t)hi * na) { const uint64_t a0 = jo[(size_t)lo * na], a1 = jo[(size_t)hi * na]; if (a1 < roff.size() && a0 <= a1) want += (size_t)((roff[a1] - roff[a0]) * 7 / 2) + (size_t)(a1 - a0) * 600; }
      text = part_take(want + want / 16);
    }
    std::vector<std::string> cigars, mds;
    std::vector<uint64_t> alnOf;                                          // piece mode: the alignment of every record
    std::vector<lra_aln_record> recs;
    std::vector<int32_t> seg_off, index;
    std::vector<lra_aln_group> groups;
    std::vector<char> buf;
    std::string rcRead;
    int rc = LRA_OK, r = lo;
    for (; r < hi; r++) {
      recs.clear(); cigars.clear(); mds.clear(); seg_off.assign(1, 0); rcRead.clear(); alnOf.clear();
      if (PT) ppart[tix].first.push_back(ppart[tix].pieces.size());
      const bool flagged = !rstat.empty() && rstat[r];
      if (flagged && (!o->flagged_unaligned || (rstat[r] & LRA_ST_DEFERRED))) { plen[tix].push_back(0); continue; }   // flagged read: no record (the caller routes it elsewhere; d_read_status, lra_map_host_flagged)
      // low-accuracy path: p == 0 left no SegAlignment (Map_lowacc.h:578-581); high-accuracy path: read.unaligned or alignments.size() == 0
      // (Map_highacc.h:778-781) = no chain of the read got its SegAlignmentGroup
      bool unaligned = flagged || nJ == 0 || jo[(size_t)r * na + 1] == jo[(size_t)r * na];   // (opts.flagged_unaligned: a flagged read is written as an unaligned one)
      bool sparseRead = false;                                            // the read took the REFINEclusters branch: smallOpts.globalK = glIndex.k (Map_highacc.h:430)
      if (hi && nJ && !flagged) {
        unaligned = true;
        for (int p = 0; p < na; p++) if (!reached.empty() && reached[(size_t)r * na + p]) { unaligned = false; sparseRead |= (reached[(size_t)r * na + p] & 2) != 0; }
      }
      if (!unaligned) {
        size_t total = 0;
        for (int p = 0; p < na; p++) total += (size_t)(jo[(size_t)r * na + p + 1] - jo[(size_t)r * na + p]);
        cigars.reserve(total);                                            // the records keep pointers into these strings
        if (withMd) mds.reserve(total);
        for (int p = 0; p < na; p++) {
          const size_t j = (size_t)r * na + p;
          // a chain that never reaches :574 ends the loop over p (:267, :491); one that does keeps its (possibly empty) group (:574-600)
          // (on the high-accuracy path a chain without clusters is skipped, Map_highacc.h:697, and the loop goes on)
          if (!reached.empty() ? !reached[j] : jo[j + 1] == jo[j]) { if (hi) continue; break; }
          for (uint64_t a = jo[j]; a < jo[j + 1]; a++) {
            // (a 30 kb read at 10 % error has ~6000 runs, nearly all of one or two digits: written through a pointer into room for the longest form, not appended one
            // by one -- the CIGAR strings were two thirds of the record threads' time)
            std::string cg;
            const size_t nRuns = PT ? 0 : (size_t)(roff[a + 1] - roff[a]);     // (piece mode: the CIGAR text is the device's)
            cg.resize(nRuns * 11 + 1);
            char* w = &cg[0];
            for (uint64_t x = roff[a]; x < roff[a] + nRuns; x++) {
              uint32_t v = runs[x] >> 4;
              if (v < 10) *w++ = (char)('0' + v);
              else if (v < 100) { *w++ = (char)('0' + v / 10); *w++ = (char)('0' + v % 10); }
              else { char tmp[12]; int k = 12; do { tmp[--k] = (char)('0' + v % 10); v /= 10; } while (v); memcpy(w, tmp + k, (size_t)(12 - k)); w += 12 - k; }
              *w++ = "=XID"[runs[x] & 15];
            }
            cg.resize((size_t)(w - &cg[0]));
            cigars.push_back(std::move(cg));
            const int32_t* c = &counts[18 * a];
            lra_aln_record rec; memset(&rec, 0, sizeof rec);
            rec.read_name = names[r]; rec.read = reads ? reads[r] : nullptr; rec.qual = quals ? quals[r] : nullptr; rec.read_len = read_len[r];
            rec.chrom = chrom_names[chrom[a]]; rec.genome_len = (uint32_t)(h->chrom_pos[chrom[a] + 1] - h->chrom_pos[chrom[a]]);
            rec.cigar = cigars.back().c_str();
            rec.strand = strand[a]; rec.supplementary = supp[a]; rec.is_secondary = sec[a];
            rec.nm = c[0]; rec.nmm = c[1]; rec.nins = c[2]; rec.ndel = c[3]; rec.tdel = c[4]; rec.tins = c[5]; rec.nSmallDel = c[6]; rec.nMedDel = c[7]; rec.nLargeDel = c[8];
            rec.nSmallIns = c[9]; rec.nMedIns = c[10]; rec.nLargeIns = c[11]; rec.pre_clip = c[12]; rec.suf_clip = c[13];
            rec.q_start = (uint32_t)c[14]; rec.q_end = (uint32_t)c[15]; rec.t_start = (uint32_t)c[16]; rec.t_end = (uint32_t)c[17];
            rec.value = fval[a]; rec.NumOfAnchors0 = n0[a]; rec.NumOfAnchors1 = n1[a];
            const uint64_t b0 = boff[a], b1 = boff[a + 1];
            rec.n_blocks = (int32_t)(b1 - b0);
            rec.first_block_qpos = ends[2 * a];
            rec.last_block_qend = ends[2 * a + 1];
            // Alignment::read is the strand the segment lies on: strands[str] (the constructor call Map_lowacc.h:560 / Map_highacc.h:704, UpdateParameters Alignment.h:506-507),
            // so a reverse-strand record's SEQ is the read's reverse complement (its quality string stays as it came, Alignment.h:717-733).  Rounds 1-5 wrote the read as
            // it came for both strands: the emitters were pinned with the read they were GIVEN, and nothing pinned which read the composition gives them.
            if (strand[a] && rcRead.empty() && !PT) {                     // CreateRC (SeqUtils.h:151); piece mode: the strands are the device's
              const int L = read_len[r];
              rcRead.resize((size_t)L);
              for (int x = 0; x < L; x++) {
                const char ch = reads[r][L - 1 - x];
                rcRead[x] = ch == 'A' ? 'T' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch == 'T' ? 'A' : ch == 'a' ? 't' : ch == 'c' ? 'g' : ch == 'g' ? 'c' : ch == 't' ? 'a' : ch == 'n' ? 'n' : 'N';
              }
            }
            if (strand[a]) rec.read = rcRead.c_str();
            if (withMd && PT) rec.md = "";                               // (the value is a piece)
            else if (withMd) {                                            // opts.printMD: PrintSAM's MD:Z (Alignment.h:763-767)
              mds.emplace_back(h->md.data() + h->md_off[a], (size_t)(h->md_off[a + 1] - h->md_off[a]));
              rec.md = mds.back().c_str();
            }
            if (pairwise) {
              rec.blocks = &blocks[3 * b0];
              rec.strand_read = strand[a] ? rcRead.c_str() : reads[r];
              rec.chrom_text = h->segText[a].data() - h->segStart[a];     // chrom_text[tPos] for the covered tPos only
            }
            recs.push_back(rec);
            if (PT) alnOf.push_back(a);
          }
          seg_off.push_back((int32_t)recs.size());
        }
      }
      uint64_t need = 0;
      if (hi && !unaligned && recs.empty()) need = 0;                     // OUTPUT prints nothing: groups exist, the first has no segment, read.unaligned == 0 (Mapping_ultility.h:467-492)
      else if (unaligned || recs.empty()) {
        lra_aln_record un; memset(&un, 0, sizeof un);
        un.read_name = names[r]; un.read = reads ? reads[r] : nullptr; un.qual = quals ? quals[r] : nullptr; un.read_len = read_len[r];
        const size_t before = text.size();
        if (PT) {
          lra_piece_sink k{ppart[tix], ppart[tix].pieces.size(), nullptr, nullptr, (uint32_t)r, read_len[r]};
          if ((rc = piece_output_read(nullptr, nullptr, 0, nullptr, o->PrintNumAln, pieceFormat, o->hardClip, tags ? tags[r] : passthrough, &un, k))) break;
        } else
        if ((rc = lra_output_read_str(nullptr, nullptr, 0, nullptr, o->PrintNumAln, (char)o->printFormat, o->hardClip, tags ? tags[r] : passthrough, 1, &un, text))) break;
        need = text.size() - before;
      } else {
        const int n = (int)seg_off.size() - 1;
        groups.assign(n, lra_aln_group()); index.assign(n, 0);
        if ((rc = lra_group_alignments(recs.data(), seg_off.data(), n, groups.data())) || (rc = lra_order_alignments(groups.data(), n, recs.data(), index.data(), 0)) ||
            (rc = lra_simple_mapqv(groups.data(), index.data(), n, recs.data(), o->bypassClustering, o->readType == LRA_READ_CLR, o->readType == LRA_READ_ONT,
                                   (hi && !sparseRead) ? o->globalK : o->localK)))                         // SimpleMapQV(alignmentsOrder, read, smallOpts): smallOpts.globalK = glIndex.k (Map_lowacc.h:233, :610); = opts.globalK on the high-accuracy path (Map_highacc.h:402, :736)
          break;
        // (the records' text goes straight into the thread's part, written once: the sizing-then-filling calls of the C entry points formatted every record four times)
        const size_t before = text.size();
        if (PT) {
          lra_piece_sink k{ppart[tix], ppart[tix].pieces.size(), recs.data(), alnOf.data(), (uint32_t)r, read_len[r], chrom.data(), roff.data(), PT->cigar_limit};
          if ((rc = piece_output_read(groups.data(), index.data(), n, recs.data(), o->PrintNumAln, pieceFormat, o->hardClip, tags ? tags[r] : passthrough, nullptr, k))) break;
        } else
        if ((rc = lra_output_read_str(groups.data(), index.data(), n, recs.data(), o->PrintNumAln, (char)o->printFormat, o->hardClip, tags ? tags[r] : passthrough, 0, nullptr, text))) break;
        need = text.size() - before;
      }
      plen[tix].push_back(need);
    }
    prc[tix] = rc;
    if (rc) pbad[tix] = r;
  };
  const bool rdbg = getenv("LRA_RECORD_DBG") != nullptr;
  auto wallr = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double tr0 = wallr();
  if (T == 1) work(0);
  else {
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++) th.emplace_back(work, t);
    for (auto& x : th) x.join();
  }
  if (rdbg) fprintf(stderr, "[records] %d threads: per-read work %.0f ms\n", T, wallr() - tr0);
  for (int t = 0; t < T; t++) if (prc[t]) { if (PT) PT->bad_read = pbad[t]; return prc[t]; }
  if (PT) {                                                              // the ranges' pieces joined in read order; a literal's place moves with its range's blob
    size_t np = 0, nb = 0;
    for (int t = 0; t < T; t++) { np += ppart[t].pieces.size(); nb += ppart[t].blob.size(); }
    PT->pieces.clear(); PT->pieces.reserve(np); PT->blob.clear(); PT->blob.reserve(nb); PT->read_piece.clear(); PT->read_piece.reserve((size_t)n_reads + 1);
    for (int t = 0; t < T; t++) {
      const uint64_t p0 = PT->pieces.size(), b0 = PT->blob.size();
      for (uint64_t f : ppart[t].first) PT->read_piece.push_back(p0 + f);
      const uint64_t s0 = PT->seq.size(), q0 = PT->qual.size();
      for (lra_rec_piece q : ppart[t].pieces) {
        if (q.kind == LRA_PIECE_LIT) q.src += b0; else if (q.kind == LRA_PIECE_BAM_SEQ) q.src += s0; else if (q.kind == LRA_PIECE_BAM_QUAL) q.src += q0;
        PT->pieces.push_back(q);
      }
      PT->blob += ppart[t].blob;
      for (uint64_t f : ppart[t].rec_first) PT->rec_first.push_back(p0 + f);
      PT->seq.insert(PT->seq.end(), ppart[t].seq.begin(), ppart[t].seq.end());
      PT->qual.insert(PT->qual.end(), ppart[t].qual.begin(), ppart[t].qual.end());
    }
    PT->read_piece.push_back(PT->pieces.size());
    PT->rec_first.push_back(PT->pieces.size());
    *len = 0;
    return LRA_OK;
  }
  // the ranges' texts joined in read order: every thread copies its own part to its place (the pages of the joined text are first touched by 256 threads, not one)
  lra_text_buf& out = h->text;
  std::vector<size_t> pstart((size_t)T + 1, 0);
  for (int t = 0; t < T; t++) pstart[t + 1] = pstart[t] + part[t].size();
  out.alloc(pstart[T]);
  if (pstart[T] && !out.data()) return LRA_ERR_NOMEM;
  h->rec_off.assign((size_t)n_reads + 1, 0);
  uint64_t at = 0; size_t r = 0;
  for (int t = 0; t < T; t++) for (uint64_t l : plen[t]) { h->rec_off[r++] = at; at += l; }
  h->rec_off[n_reads] = at;
  {
    auto copy = [&](int t) { if (!part[t].empty()) memcpy(out.data() + pstart[t], part[t].data(), part[t].size()); part_give(part[t]); };
    if (T == 1) copy(0);
    else { std::vector<std::thread> th; for (int t = 0; t < T; t++) th.emplace_back(copy, t); for (auto& x : th) x.join(); }
  }
  *len = out.size();
  if (text) *text = out.data();
  if (rec_off) *rec_off = h->rec_off.data();
  if (rdbg) fprintf(stderr, "[records] joined at %.0f ms (%.2f GB)\n", wallr() - tr0, out.size() / 1e9);
  return LRA_OK;
}

extern "C" int lra_map_records_host(lra_map_host* h, const lra_map_opts* o, const char* const* names, const char* const* reads, const char* const* quals,
                                    const int32_t* read_len, const char* const* chrom_names, const char* passthrough, int n_threads, const char** text,
                                    uint64_t* len, const uint64_t** rec_off) {
  return records_host(h, o, names, reads, quals, read_len, chrom_names, passthrough, nullptr, n_threads, text, len, rec_off);
}

extern "C" int lra_map_records_host_tags(lra_map_host* h, const lra_map_opts* o, const char* const* names, const char* const* reads, const char* const* quals,
                                         const int32_t* read_len, const char* const* chrom_names, const char* const* passthrough, int n_threads,
                                         const char** text, uint64_t* len, const uint64_t** rec_off) {
  if (!passthrough) return LRA_ERR_INVALID;
  return records_host(h, o, names, reads, quals, read_len, chrom_names, nullptr, passthrough, n_threads, text, len, rec_off);
}

// MapRead's svsigstrm: Printsvsig's lines (Alignment.h:374-399) of every read, from the signatures a snapshot packed with LRA_PACK_SVSIG holds.  Host threads
// take contiguous ranges of reads, as in records_host; a read's alignments come in result order (job, then segment).
extern "C" int lra_map_svsig_host(lra_map_host* h, const char* const* names, const char* const* chrom_names, int n_threads, const char** text, uint64_t* len,
                                  const uint64_t** rec_off) {
  if (!h || !names || !chrom_names || !len || !h->has_sv) return LRA_ERR_INVALID;
  const int n_reads = h->n_reads, na = h->num_aln;
  const size_t nJ = h->nJ;
  if (nJ && (h->jo.size() != nJ + 1 || nJ != (size_t)n_reads * na || h->jo[nJ] > h->nA)) return LRA_ERR_INVALID;
  int T = n_threads > 0 ? n_threads : lra_host_threads();
  T = std::max(1, std::min(T, n_reads / 32 + 1));
  std::vector<std::string> part(T);
  std::vector<std::vector<uint64_t>> plen(T);
  auto put_num = [](std::string& s, uint64_t v) { char tmp[24]; int k = 24; do { tmp[--k] = (char)('0' + v % 10); v /= 10; } while (v); s.append(tmp + k, (size_t)(24 - k)); };
  auto work = [&](int tix) {
    const int lo = (int)((long)n_reads * tix / T), hi = (int)((long)n_reads * (tix + 1) / T);
    std::string& out = part[tix];
    plen[tix].reserve((size_t)(hi - lo));
    for (int r = lo; r < hi; r++) {
      const size_t before = out.size();
      const bool flagged = !h->rstat.empty() && h->rstat[r];                // flagged or handed back: no alignment of the read is output
      if (!flagged && nJ) {
        for (uint64_t a = h->jo[(size_t)r * na]; a < h->jo[(size_t)(r + 1) * na]; a++) {
          for (uint64_t x = h->sv_off[a]; x < h->sv_off[a + 1]; x++) {
            const lra_svsig_rec& g = h->sv_rec[x];
            out += chrom_names[h->chrom[a]]; out += '\t'; out += names[r]; out += '\t';
            put_num(out, g.t_start); out += '\t';
            put_num(out, g.kind == LRA_SV_DEL ? (uint32_t)(g.t_start + g.len - 1) : g.t_start); out += '\t';
            put_num(out, g.len);
            out += g.kind == LRA_SV_DEL ? "\tDEL\t" : "\tINS\t";
            out.append(h->sv_seq.data() + g.seq_off, g.len);
            out += '\n';
          }
        }
      }
      plen[tix].push_back(out.size() - before);
    }
  };
  if (T == 1) work(0);
  else { std::vector<std::thread> th; for (int t = 0; t < T; t++) th.emplace_back(work, t); for (auto& x : th) x.join(); }
  size_t total = 0;
  for (int t = 0; t < T; t++) total += part[t].size();
  h->sv_text.alloc(total);
  if (total && !h->sv_text.data()) return LRA_ERR_NOMEM;
  h->sv_rec_off.assign((size_t)n_reads + 1, 0);
  uint64_t at = 0; size_t r = 0;
  for (int t = 0; t < T; t++) {
    if (!part[t].empty()) memcpy(h->sv_text.data() + at, part[t].data(), part[t].size());
    for (uint64_t l : plen[t]) { h->sv_rec_off[r++] = at; at += l; }
  }
  h->sv_rec_off[n_reads] = at;
  *len = total;
  if (text) *text = h->sv_text.data();
  if (rec_off) *rec_off = h->sv_rec_off.data();
  return LRA_OK;
}

extern "C" int lra_map_svsig(lra_ctx* ctx, const lra_map_result* res, const char* const* names, const char* const* chrom_names, const char** text, uint64_t* len,
                             const uint64_t** rec_off) {
  if (!ctx || !res || !names || !chrom_names || !len || !ctx->map) return LRA_ERR_INVALID;
  lra_map_host* h = nullptr;
  int rc = lra_map_snapshot(ctx, res, LRA_PACK_SVSIG, &h);
  if (rc) return rc;
  if (!(rc = lra_map_svsig_host(h, names, chrom_names, 0, nullptr, len, nullptr))) {
    lra_map_state* m = ctx->map;                                           // the text outlives the snapshot: the context keeps it until the next call
    m->sv_text.swap(h->sv_text); m->sv_off.swap(h->sv_rec_off);
    if (text) *text = m->sv_text.data();
    if (rec_off) *rec_off = m->sv_off.data();
  }
  lra_map_host_free(h);
  return rc;
}

static int map_records(lra_ctx* ctx, const lra_map_result* res, const lra_map_opts* o, const char* const* names, const char* const* reads,
                       const char* const* quals, const int32_t* read_len, const char* const* chrom_names, const char* passthrough, const char* const* tags,
                       char* out, uint64_t cap, uint64_t* len, uint64_t* rec_off) {
  if (!ctx || !res || !o || !names || !reads || !read_len || !chrom_names || !len) return LRA_ERR_INVALID;
  lra_map_state* m = ctx->map;
  if (!m) return LRA_ERR_INVALID;
  // two-call convention: the sizing call keeps its text, the filling call for the same result and format hands it over (per-read tags: their array
  // stands where the one passthrough text does)
  const lra_map_sig sig{res->d_blocks, res->d_runs, res->n_reads, res->n_alignments, o->printFormat, o->PrintNumAln, o->hardClip,
                        tags ? (const char*)tags : passthrough, o->flagged_unaligned, res->d_read_status};
  if (out && m->last_sig == sig && !m->last_text.empty() && cap >= m->last_text.size()) {
    memcpy(out, m->last_text.data(), m->last_text.size());
    *len = m->last_text.size();
    if (rec_off) memcpy(rec_off, m->last_off.data(), m->last_off.size() * 8);
    m->last_text.clear(); m->last_sig = lra_map_sig{};
    return LRA_OK;
  }
  lra_map_host* h = nullptr;
  int rc = lra_map_snapshot(ctx, res, o->printFormat == 'a', &h);
  if (rc) return rc;
  const char* text = nullptr; const uint64_t* ro = nullptr;
  rc = records_host(h, o, names, reads, quals, read_len, chrom_names, passthrough, tags, 0, &text, len, &ro);
  if (rc) { lra_map_host_free(h); return rc; }
  if (rec_off) memcpy(rec_off, ro, ((size_t)res->n_reads + 1) * 8);
  if (!out) {                                                            // sizing call: remember text and offsets
    m->last_text.swap(h->text); m->last_off.swap(h->rec_off); m->last_sig = sig;
    lra_map_host_free(h);
    return LRA_OK;
  }
  m->last_sig = lra_map_sig{};
  if (cap < *len) { lra_map_host_free(h); return LRA_ERR_INVALID; }
  memcpy(out, text, *len);
  lra_map_host_free(h);
  return LRA_OK;
}

extern "C" int lra_map_records(lra_ctx* ctx, const lra_map_result* res, const lra_map_opts* o, const char* const* names, const char* const* reads,
                               const char* const* quals, const int32_t* read_len, const char* const* chrom_names, const char* passthrough, char* out,
                               uint64_t cap, uint64_t* len, uint64_t* rec_off) {
  return map_records(ctx, res, o, names, reads, quals, read_len, chrom_names, passthrough, nullptr, out, cap, len, rec_off);
}

extern "C" int lra_map_records_tags(lra_ctx* ctx, const lra_map_result* res, const lra_map_opts* o, const char* const* names, const char* const* reads,
                                    const char* const* quals, const int32_t* read_len, const char* const* chrom_names, const char* const* passthrough,
                                    char* out, uint64_t cap, uint64_t* len, uint64_t* rec_off) {
  if (!passthrough) return LRA_ERR_INVALID;
  return map_records(ctx, res, o, names, reads, quals, read_len, chrom_names, nullptr, passthrough, out, cap, len, rec_off);
}

// ---- the record text built on the device (records.hip) ---------------------------------------------------------------------------------------------
// LRA_PACK_SVSIG of the device formats: the signatures (svsig.hip) and their text (svsig_text.hip) from the result's own arrays; adr = k_md_address's offsets.
// The host's part is the two name tables, uploaded as one buffer: offsets u64[n_reads + 1] | offsets u64[n_chrom + 1] | the read names | the chromosome names.
static int records_device_svsig(lra_ctx* ctx, const lra_map_result* res, const uint64_t* adr, const char* const* names, const char* const* chrom_names,
                                lra_records_device_stats& S) {
  lra_map_state* m = ctx->map;
  hipStream_t st = ctx->stream;
  const int nR = res->n_reads, na = std::max(res->num_aln, 1);
  const uint64_t nA = res->n_alignments, nJ = res->n_jobs;
  const double t0 = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
  m->dev_sv_off.assign((size_t)nR + 1, 0);
  m->dev_sv_ptr = nullptr; m->dev_sv_len = 0;
  if (nA && nJ) {
    if (nJ != (uint64_t)nR * na || !res->d_job_aln_off) return lra_set_err(ctx, LRA_ERR_INVALID, "LRA_PACK_SVSIG: the result's jobs are not its reads'");
    int rc;
    lra_svsig_result sv; memset(&sv, 0, sizeof sv);
    if ((rc = lra_sv_signatures_batch(ctx, (int)nA, res->d_blocks, res->d_block_off, res->d_strands, adr, nullptr, (const char*)ctx->seed->genome, adr + nA + 1,
                                      ctx->svsig_len, &sv))) return rc;
    S.svsig_bytes_d2h += 24;                                             // (its block count and two totals)
    if (sv.n_sig) {
      const size_t nCh = m->chrom_pos.size() - 1;
      std::vector<uint64_t> off((size_t)nR + 1 + nCh + 1, 0);
      for (int r = 0; r < nR; r++) off[(size_t)r + 1] = off[r] + strlen(names[r]);
      uint64_t* coff = off.data() + nR + 1;
      for (size_t c = 0; c < nCh; c++) coff[c + 1] = coff[c] + strlen(chrom_names[c]);
      const size_t offBytes = off.size() * 8, rBytes = (size_t)off[nR], cBytes = (size_t)coff[nCh], up = offBytes + rBytes + cBytes;
      char* stage = (char*)lra_pinned(ctx, up);
      // scratch 1 (dead at return; lra_svsig_text_batch works in scratch 0): the name tables, the skip bytes, rec_off
      const size_t upPad = (up + 64 + 255) & ~(size_t)255, skipPad = (nA + 255) & ~(size_t)255;
      char* dev = (char*)lra_scratch(ctx, 1, upPad + skipPad + ((size_t)nR + 1) * 8);
      if (!stage || !dev) return LRA_ERR_NOMEM;
      char* w = dev + upPad;
      memcpy(stage, off.data(), offBytes);
      for (int r = 0; r < nR; r++) memcpy(stage + offBytes + off[r], names[r], (size_t)(off[(size_t)r + 1] - off[r]));
      for (size_t c = 0; c < nCh; c++) memcpy(stage + offBytes + rBytes + coff[c], chrom_names[c], (size_t)(coff[c + 1] - coff[c]));
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(dev, stage, up, hipMemcpyHostToDevice, st));
      S.svsig_bytes_h2d += up;
      uint8_t* skip = nullptr;
      if (res->d_read_status) {
        skip = (uint8_t*)w;
        hipLaunchKernelGGL(k_sv_skip, dim3((unsigned)((nA + 255) / 256)), dim3(256), 0, st, nA, nR, res->d_aln_read, res->d_read_status, skip);
      }
      uint64_t* d_rec_off = (uint64_t*)(w + skipPad);
      LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));                      // (the staging buffer is free again)
      const uint64_t* d_roff = (const uint64_t*)dev; const uint64_t* d_coff = d_roff + nR + 1;
      lra_svsig_text_result tx; memset(&tx, 0, sizeof tx);
      if ((rc = lra_svsig_text_batch(ctx, &sv, res->d_aln_read, res->d_chrom, skip, nR, dev + offBytes, d_roff, (int)nCh, dev + offBytes + rBytes, d_coff, &tx))) return rc;
      S.svsig_bytes_d2h += 8;
      if (tx.n_bytes) {
        if (ctx->sv_pin_bytes < tx.n_bytes) {                            // kept and grown as the record text's buffer is
          if (ctx->sv_pin) { (void)hipHostFree(ctx->sv_pin); ctx->sv_pin = nullptr; ctx->sv_pin_bytes = 0; }
          const size_t want = tx.n_bytes + tx.n_bytes / 4 + 4096;
          if (hipHostMalloc(&ctx->sv_pin, want, hipHostMallocDefault) != hipSuccess) { ctx->sv_pin = nullptr; return lra_set_err(ctx, LRA_ERR_NOMEM, "hipHostMalloc(%zu) failed", want); }
          ctx->sv_pin_bytes = want;
        }
        hipLaunchKernelGGL(k_sv_rec_off, dim3((unsigned)(((size_t)nR + 1 + 255) / 256)), dim3(256), 0, st, nR, na, nJ, nA, res->d_job_aln_off, tx.d_aln_off, d_rec_off);
        LRA_HIP_CHECK(ctx, hipMemcpyAsync(m->dev_sv_off.data(), d_rec_off, ((size_t)nR + 1) * 8, hipMemcpyDeviceToHost, st));
        LRA_HIP_CHECK(ctx, hipMemcpyAsync(ctx->sv_pin, tx.d_text, tx.n_bytes, hipMemcpyDeviceToHost, st));
        LRA_HIP_CHECK(ctx, hipGetLastError());
        LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
        S.svsig_bytes_d2h += tx.n_bytes + ((size_t)nR + 1) * 8;
        m->dev_sv_ptr = (const char*)ctx->sv_pin; m->dev_sv_len = tx.n_bytes;
      }
    }
  }
  S.svsig_text_bytes = m->dev_sv_len;
  S.ms_svsig = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count() - t0;
  m->dev_sv = true;
  return LRA_OK;
}

// The host half: a snapshot without the runs, the piece table on host threads; the device half: the CIGAR text, MD, the pairwise rows, the assembly.  See lra_hip.h.
// keep: the device formats' text stays on the device (*text is a device pointer then), for lra_map_records_device_bgzf
static int records_device(lra_ctx* ctx, const lra_map_result* res, const lra_map_opts* o, const char* const* names, const char* const* reads,
                          const char* const* quals, const int32_t* read_len, const char* const* chrom_names, const char* const* passthrough,
                          const char* d_qual, const uint64_t* d_qual_off, int flags, int n_threads, const char** text, uint64_t* len,
                          const uint64_t** rec_off, bool keep, bool bam = false, const uint64_t** d_rec_start = nullptr, uint64_t* n_rec = nullptr) {
  if (!ctx || !res || !o || !names || !read_len || !chrom_names || !len || (flags & ~(LRA_PACK_MD | LRA_PACK_SVSIG)) || (d_qual && !d_qual_off)) return LRA_ERR_INVALID;
  lra_map_state* m = ctx->map;
  if (!m) return LRA_ERR_INVALID;
  if (bam && o->printFormat != 's') return lra_set_err(ctx, LRA_ERR_INVALID, "lra_map_records_device_bam: print format '%c' has no BAM form (only 's')", (char)o->printFormat);
  m->dev_sv = false;
  const bool withSv = (flags & LRA_PACK_SVSIG) != 0;
  m->dev_stats = lra_records_device_stats{};
  lra_records_device_stats& S = m->dev_stats;
  auto wall = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const int nR = res->n_reads;
  const bool pairwise = o->printFormat == 'a';
  const bool device = o->printFormat == 's' || o->printFormat == 'P' || pairwise;
  lra_map_host* h = nullptr;
  int rc;
  if (!device) {                                                         // 'p', 'b': no long field worth moving -- the host path, its text kept by the context
    if (!reads) return LRA_ERR_INVALID;
    if ((rc = lra_map_snapshot(ctx, res, flags & (LRA_PACK_MD | LRA_PACK_SVSIG), &h))) return rc;
    const char* t = nullptr; const uint64_t* ro = nullptr;
    rc = records_host(h, o, names, reads, quals, read_len, chrom_names, nullptr, passthrough, n_threads, &t, len, &ro);
    uint64_t svLen = 0;
    if (!rc && withSv) rc = lra_map_svsig_host(h, names, chrom_names, n_threads, nullptr, &svLen, nullptr);
    if (!rc) {
      m->dev_text.swap(h->text); m->dev_off.swap(h->rec_off);
      if (text) *text = m->dev_text.data();
      if (rec_off) *rec_off = m->dev_off.data();
      if (withSv) {
        m->dev_sv_text.swap(h->sv_text); m->dev_sv_off.swap(h->sv_rec_off);
        m->dev_sv_ptr = m->dev_sv_text.data(); m->dev_sv_len = svLen; m->dev_sv = true;
      }
    }
    lra_map_host_free(h);
    return rc;
  }
  double t0 = wall();
  if ((rc = lra_map_snapshot(ctx, res, LRA_PACK_NORUNS, &h))) return rc;
  std::unique_ptr<lra_map_host> hold(h);
  const uint64_t nA = h->nA;
  S.bytes_d2h += PackLayout(nR, h->nJ, nA, 0, 0, h->chrom_pos.size() - 1).total;
  double t1 = wall();
  S.ms_snapshot = t1 - t0;
  // the long fields the alignments own: the CIGAR text, and with LRA_PACK_MD the MD:Z values (as lra_map_pack makes them); format 'a': the pairwise rows
  const bool withMd = (flags & LRA_PACK_MD) && o->printFormat == 's';
  lra_cigar_text_result cg; memset(&cg, 0, sizeof cg);
  lra_md_result md; memset(&md, 0, sizeof md);
  lra_pairwise_text_result pw; memset(&pw, 0, sizeof pw);
  hipStream_t st = ctx->stream;
  uint64_t* adr = nullptr;
  if (nA) {
    if (!res->d_run_off || !res->d_strands) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_map_records_device: the result has no runs / reads to work on");
    // (BAM records: the CIGAR text is SA:Z's only -- made below, once the piece table says a record names it)
    if (!pairwise && !bam && (rc = lra_cigar_text_batch(ctx, (int)nA, res->d_runs, res->d_run_off, nullptr, nullptr, nullptr, &cg))) return rc;
    if (withMd || pairwise || withSv) {
      if (!res->d_aln_read || !res->d_strand || !res->d_chrom || !res->d_blocks || !res->d_block_off)
        return lra_set_err(ctx, LRA_ERR_INVALID, "lra_map_records_device: the result has no blocks to work on");
      if (!ctx->seed || !ctx->seed->genome || !m->d_chrom_pos) return lra_set_err(ctx, LRA_ERR_INVALID, "LRA_PACK_MD / LRA_PACK_SVSIG / print format 'a': genome not loaded");
      adr = (uint64_t*)lra_ensure(ctx, 187, 2 * (nA + 1) * 8);
      if (!adr) return LRA_ERR_NOMEM;
      const uint64_t* ro = (const uint64_t*)(res->d_strands + lra_strands_ro_at(res->rc_base));
      hipLaunchKernelGGL(k_md_address, dim3((unsigned)((nA + 255) / 256)), dim3(256), 0, st, nA, res->d_aln_read, res->d_strand, res->d_chrom, ro, res->rc_base,
                         (const uint64_t*)m->d_chrom_pos, adr, adr + nA + 1);
      if (withMd && (rc = lra_md_strings_batch(ctx, (int)nA, res->d_blocks, res->d_block_off, res->d_strands, adr, nullptr, (const char*)ctx->seed->genome, adr + nA + 1, &md))) return rc;
      if (pairwise && (rc = lra_pairwise_text_batch(ctx, (int)nA, res->d_blocks, res->d_block_off, res->d_strands, adr, nullptr, (const char*)ctx->seed->genome, adr + nA + 1, &pw))) return rc;
    }
  }
  double t2 = wall();
  S.ms_cigar_md = t2 - t1;
  lra_piece_table PT;
  PT.bam = bam; PT.cigar_limit = ctx->bam_cigar_limit;
  uint64_t dummy = 0;
  if ((rc = records_host(h, o, names, reads, quals, read_len, chrom_names, nullptr, passthrough, n_threads, nullptr, &dummy, nullptr, &PT, withMd))) {
    if (bam && rc == LRA_ERR_INVALID && PT.bad_read >= 0 && PT.bad_read < nR)
      return lra_set_err(ctx, rc, "lra_map_records_device_bam: read %d (%.64s): %s", PT.bad_read, names[PT.bad_read],
                         strlen(names[PT.bad_read]) > 254 ? "a name above 254 bytes" : "its passthrough text is not SAM aux fields");
    return rc;
  }
  double t3 = wall();
  S.ms_pieces = t3 - t2;
  // BAM records: the three staging arrays.  The ranges and requests go up in work buffer 75, the ranges with the device's own read offsets.
  lra_bam_cigar_result bcg; memset(&bcg, 0, sizeof bcg);
  lra_bam_bytes_result bsq; memset(&bsq, 0, sizeof bsq);
  lra_bam_bytes_result bph; memset(&bph, 0, sizeof bph);
  const lra_bam_qual_req* d_req = nullptr;
  if (bam) {
    const size_t nS = PT.seq.size(), nQ = PT.qual.size();
    bool saCigar = false;
    for (const lra_rec_piece& p : PT.pieces) if (p.kind == LRA_PIECE_CIGAR) { saCigar = true; break; }
    if (nA && saCigar && (rc = lra_cigar_text_batch(ctx, (int)nA, res->d_runs, res->d_run_off, nullptr, nullptr, nullptr, &cg))) return rc;
    if (nA && (rc = lra_bam_cigar_batch(ctx, (int)nA, res->d_runs, res->d_run_off, nullptr, nullptr, nullptr, &bcg))) return rc;
    if (nS && !res->d_strands) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_map_records_device_bam: the result has no reads to work on");
    const size_t sBytes = (nS * sizeof(lra_bam_seq_range) + 255) & ~(size_t)255, qBytes = nQ * sizeof(lra_bam_qual_req);
    char* up = (char*)lra_ensure(ctx, 75, sBytes + qBytes + 64);
    if (!up) return LRA_ERR_NOMEM;
    if (nS) {
      std::vector<uint64_t> ro((size_t)nR + 1);
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(ro.data(), res->d_strands + lra_strands_ro_at(res->rc_base), ((size_t)nR + 1) * 8, hipMemcpyDeviceToHost, st));
      LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
      S.bytes_d2h += ((size_t)nR + 1) * 8;
      for (lra_bam_seq_range& q : PT.seq) {
        const uint64_t r = (q.off >> 32) & 0x7fffffffu, from = q.off & 0xffffffffu;
        q.off = ro[r] + from + ((q.off >> 63) ? res->rc_base : 0);
      }
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(up, PT.seq.data(), nS * sizeof(lra_bam_seq_range), hipMemcpyHostToDevice, st));
    }
    if (nQ) LRA_HIP_CHECK(ctx, hipMemcpyAsync(up + sBytes, PT.qual.data(), qBytes, hipMemcpyHostToDevice, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    S.bytes_h2d += nS * sizeof(lra_bam_seq_range) + qBytes;
    d_req = (const lra_bam_qual_req*)(up + sBytes);
    // (both strands of the batch lie in [0, 2 * rc_base): a range is cut to the read on the host, so it lies inside)
    if ((rc = lra_bam_pack_seq_batch(ctx, nS, (const lra_bam_seq_range*)up, (const uint8_t*)res->d_strands, 2 * res->rc_base, &bsq))) return rc;
    S.ms_cigar_md += wall() - t3;
    t3 = wall();
  }
  // the qualities: the caller's device copy, or the strings of the reads that print them, uploaded through the context's page-locked staging
  const char* dq = d_qual; const uint64_t* dqo = d_qual_off;
  if (!dq) {
    std::vector<uint64_t> qo((size_t)nR + 1, 0);
    bool any = false;
    for (const lra_rec_piece& p : PT.pieces)                             // (a string shorter than its read -- "*" -- is uploaded as far as it goes; the device cuts the piece to it)
      if (p.kind == LRA_PIECE_QUAL) { const size_t r = (size_t)(p.src >> 32); qo[r + 1] = strnlen(quals[r], (size_t)std::max(read_len[r], 0)); any = true; }
    for (const lra_bam_qual_req& q : PT.qual)                            // (BAM records: the same strings, named by the requests)
      if (q.read < (uint32_t)nR && quals && quals[q.read]) { qo[(size_t)q.read + 1] = strnlen(quals[q.read], (size_t)std::max(read_len[q.read], 0)); any = true; }
    if (any) {
      for (int r = 0; r < nR; r++) qo[(size_t)r + 1] += qo[r];
      const size_t offBytes = ((size_t)nR + 1) * 8, total = (size_t)qo[nR];
      char* stage = (char*)lra_pinned(ctx, offBytes + total);
      char* dev = (char*)lra_ensure(ctx, 169, offBytes + total + 64);
      if (!stage || !dev) return LRA_ERR_NOMEM;
      memcpy(stage, qo.data(), offBytes);
      for (int r = 0; r < nR; r++) if (qo[(size_t)r + 1] > qo[r]) memcpy(stage + offBytes + qo[r], quals[r], (size_t)(qo[(size_t)r + 1] - qo[r]));
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(dev, stage, offBytes + total, hipMemcpyHostToDevice, st));
      LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
      dqo = (const uint64_t*)dev; dq = dev + offBytes;
      S.bytes_h2d += offBytes + total;
    }
  }
  S.ms_upload = wall() - t3;
  if (bam) {
    const double tq = wall();
    if ((rc = lra_bam_phred_batch(ctx, PT.qual.size(), d_req, nR, dq, dqo, &bph))) return rc;
    S.ms_cigar_md += wall() - tq;
  }
  lra_rec_job J;
  J.n_reads = nR; J.n_aln = nA; J.pieces = PT.pieces.data(); J.n_pieces = PT.pieces.size(); J.read_piece = PT.read_piece.data();
  J.blob = PT.blob.data(); J.blob_bytes = PT.blob.size();
  J.d_strands = res->d_strands; J.rc_base = res->rc_base;
  J.d_read_off = res->d_strands ? (const uint64_t*)(res->d_strands + lra_strands_ro_at(res->rc_base)) : nullptr;
  J.d_qual = dq; J.d_qual_off = dqo; J.d_cg = cg.d_text; J.d_cg_off = cg.d_off; J.d_md = withMd ? md.d_md : nullptr; J.d_md_off = withMd ? md.d_md_off : nullptr;
  J.d_pw = pw.d_text; J.d_pw_off = pw.d_off;
  if (bam) {
    J.d_bcg = bcg.d_ops; J.d_bcg_off = bcg.d_off; J.d_pseq = bsq.d_data; J.d_pseq_off = bsq.d_off; J.n_pseq = bsq.n;
    J.d_phred = bph.d_data; J.d_phred_off = bph.d_off; J.n_phred = bph.n;
    J.rec_first = PT.rec_first.data(); J.n_rec = PT.rec_first.size() - 1;
  }
  J.keep_on_device = keep;
  if (bam && d_rec_start) { *d_rec_start = nullptr; J.d_rec_start = d_rec_start; }
  if (n_rec) *n_rec = bam ? PT.rec_first.size() - 1 : 0;
  if (!J.d_strands && nR) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_map_records_device: the result has no reads to work on");
  m->dev_off.assign((size_t)nR + 1, 0);
  m->dev_text.clear();
  if ((rc = lra_records_assemble(ctx, J, text, len, m->dev_off.data(), &S))) return rc;
  if (rec_off) *rec_off = m->dev_off.data();
  if (withSv && (rc = records_device_svsig(ctx, res, adr, names, chrom_names, S))) return rc;   // (behind the records: their long fields' buffers are done with)
  return LRA_OK;
}

extern "C" int lra_map_records_device(lra_ctx* ctx, const lra_map_result* res, const lra_map_opts* o, const char* const* names, const char* const* reads,
                                      const char* const* quals, const int32_t* read_len, const char* const* chrom_names, const char* const* passthrough,
                                      const char* d_qual, const uint64_t* d_qual_off, int flags, int n_threads, const char** text, uint64_t* len,
                                      const uint64_t** rec_off) {
  return records_device(ctx, res, o, names, reads, quals, read_len, chrom_names, passthrough, d_qual, d_qual_off, flags, n_threads, text, len, rec_off, false);
}

// lra_map_records_device whose text leaves the device as BGZF members: formats 's', 'P' and 'a' compress the device text where the assembly left it (work
// buffer 99; the SV signature text, built behind it, does not touch that buffer), the fall-through formats upload the host text first (work buffer 74)
extern "C" int lra_map_records_device_bgzf(lra_ctx* ctx, const lra_map_result* res, const lra_map_opts* o, const char* const* names, const char* const* reads,
                                           const char* const* quals, const int32_t* read_len, const char* const* chrom_names,
                                           const char* const* passthrough, const char* d_qual, const uint64_t* d_qual_off, int flags, int n_threads,
                                           const uint8_t** data, uint64_t* data_len, const uint64_t** rec_off, const uint64_t** member_off,
                                           uint64_t* n_members) {
  if (!data || !data_len || !member_off || !n_members || !o) return LRA_ERR_INVALID;
  const char* text = nullptr;
  uint64_t len = 0;
  int rc = records_device(ctx, res, o, names, reads, quals, read_len, chrom_names, passthrough, d_qual, d_qual_off, flags, n_threads, &text, &len, rec_off, true);
  if (rc) return rc;
  const bool device = o->printFormat == 's' || o->printFormat == 'P' || o->printFormat == 'a';
  const uint8_t* d_text = (const uint8_t*)text;
  if (!device && len) {
    char* up = (char*)lra_ensure(ctx, 74, len + 64);
    if (!up) return LRA_ERR_NOMEM;
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(up, text, len, hipMemcpyHostToDevice, ctx->stream));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->map->dev_stats.bytes_h2d += len;
    d_text = (const uint8_t*)up;
  }
  if ((rc = lra_bgzf_compress_device(ctx, d_text, len, data, data_len, member_off, n_members))) return rc;
  ctx->map->dev_stats.bytes_d2h += *data_len;
  return LRA_OK;
}

// lra_map_records_device's SAM records as BAM records (emit_bam.h, bam_encode.hip): raw in the page-locked record buffer, or through the BGZF stream stage
extern "C" int lra_map_records_device_bam(lra_ctx* ctx, const lra_map_result* res, const lra_map_opts* o, const char* const* names, const char* const* quals,
                                          const int32_t* read_len, const char* const* chrom_names, const char* const* passthrough, const char* d_qual,
                                          const uint64_t* d_qual_off, int flags, int n_threads, int bgzf, const uint8_t** data, uint64_t* data_len,
                                          const uint64_t** rec_off, const uint64_t** member_off, uint64_t* n_members) {
  if (!data || !data_len || !member_off || !n_members || !o) return LRA_ERR_INVALID;
  *member_off = nullptr; *n_members = 0;
  const char* text = nullptr;
  uint64_t len = 0;
  int rc = records_device(ctx, res, o, names, nullptr, quals, read_len, chrom_names, passthrough, d_qual, d_qual_off, flags, n_threads, &text, &len, rec_off, bgzf != 0, true);
  if (rc) return rc;
  if (!bgzf) { *data = (const uint8_t*)text; *data_len = len; return LRA_OK; }
  if ((rc = lra_bgzf_compress_device(ctx, (const uint8_t*)text, len, data, data_len, member_off, n_members))) return rc;
  ctx->map->dev_stats.bytes_d2h += *data_len;
  return LRA_OK;
}

// lra_map_records_device_bam's stream, left on the device and handed to a sorter (bam_sort.hip) with the record starts the assembly knows
extern "C" int lra_map_records_device_bam_to_sorter(lra_ctx* ctx, const lra_map_result* res, const lra_map_opts* o, const char* const* names,
                                                    const char* const* quals, const int32_t* read_len, const char* const* chrom_names,
                                                    const char* const* passthrough, const char* d_qual, const uint64_t* d_qual_off, int flags, int n_threads,
                                                    lra_bam_sorter* sorter, const uint64_t** rec_off) {
  if (!sorter || !o) return LRA_ERR_INVALID;
  const char* text = nullptr;
  uint64_t len = 0, nRec = 0;
  const uint64_t* d_start = nullptr;
  int rc = records_device(ctx, res, o, names, nullptr, quals, read_len, chrom_names, passthrough, d_qual, d_qual_off, flags, n_threads, &text, &len, rec_off, true, true,
                          &d_start, &nRec);
  if (rc) return rc;
  if (!len || !nRec) return LRA_OK;
  if (!d_start) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_map_records_device_bam_to_sorter: the assembly gave no record starts");
  if ((rc = lra_bam_sorter_add_device(sorter, (const uint8_t*)text, d_start, nRec)))
    return rc == LRA_ERR_NOMEM ? lra_set_err(ctx, rc, "lra_map_records_device_bam_to_sorter: the batch does not fit the sorter's budget") : rc;
  return LRA_OK;
}

// the head of a BAM file: magic, the header text, the reference table (host only; two-call convention)
extern "C" int lra_bam_header(const char* text, uint64_t text_len, int n_chrom, const char* const* chrom_names, const uint64_t* chrom_pos, uint8_t* out, uint64_t cap,
                              uint64_t* len) {
  if (!len || n_chrom < 0 || (text_len && !text) || text_len > 0x7fffffffu || (n_chrom && (!chrom_names || !chrom_pos))) return LRA_ERR_INVALID;
  std::string s;
  if (lra_bam_header_str(text, text_len, n_chrom, chrom_names, chrom_pos, s)) return LRA_ERR_INVALID;
  *len = s.size();
  if (!out) return LRA_OK;
  if (cap < s.size()) return LRA_ERR_INVALID;
  memcpy(out, s.data(), s.size());
  return LRA_OK;
}

extern "C" int lra_map_records_device_svsig(lra_ctx* ctx, const char** text, uint64_t* len, const uint64_t** rec_off) {
  if (!ctx || !len || !ctx->map || !ctx->map->dev_sv) return LRA_ERR_INVALID;
  *len = ctx->map->dev_sv_len;
  if (text) *text = ctx->map->dev_sv_ptr;
  if (rec_off) *rec_off = ctx->map->dev_sv_off.data();
  return LRA_OK;
}

extern "C" int lra_map_records_device_last(lra_ctx* ctx, lra_records_device_stats* out) {
  if (!ctx || !out || !ctx->map) return LRA_ERR_INVALID;
  *out = ctx->map->dev_stats;
  return LRA_OK;
}

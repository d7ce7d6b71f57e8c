// lra_amd/csrc/bam_merge.hip -- lra_bam_merger: up to 256 coordinate-sorted BAM files streamed into one sorted stream in bounded device memory, given back
// as BGZF members with the bytes of the .bai index (gfx950).  include/lra_hip.h has the interface, the bound rule, the budget and the index's rules.
//
// window.  Each run owns one lra_bgzf_step (zsource.h, the readers' step): a refill reads the next compressed bytes, inflates their whole members on the
// device behind the carried tail, lra_bam_launch_frame chains the block_size fields, bs_keys (bam_keys.h: the sorter's kernel) keys the whole records and
// mg_order checks that the keys do not descend, the last key of the run's previous window in front of the first.  The members of a refill are walked on
// the host first (a second read of the bytes through pread), so what the refill allocates is known and checked against the budget before it does.
// round.  The host takes the bound from the windows' last keys; mg_count, a lane per run, one binary search: the records with (key, run) <= bound.
// mg_rank, a lane per emitted record, the runs' table in LDS: the record's ordinal in its run + for every earlier run the emitted records with key <= its
// own + for every later run those with key < its own; it scatters (length, address) to that rank.  Neighbouring lanes hold neighbouring keys of one run,
// so a wave's probes walk the same few cache lines.  A scan and the project's copy pass (lra_pack_strings_launch) gather the round behind the bytes the
// last round left; bs_span gives the index's per-record fields; the whole multiples of 65280 bytes go through lra_bgzf_compress_device.
// index.  mi_mark / mi_runs / mi_windows are bam_sort.hip's bi_* kernels over one round, in stream offsets u instead of virtual offsets: chunk heads
// against the last record of the round before (carried in), the chunks' [ubeg, uend) (one that continues over the round's edge hands its end to the
// host), the resident windows by 64-bit atomicMin.  At the end the host fills the windows backward, each reference's chunks are stable-sorted by bin with
// rocprim's radix sort, u becomes a virtual offset through the complete member table and lra_bai_write writes the bytes.
#include "common.h"
#include "chunk_copy.h"
#include "scan.h"
#include "bgzf_deflate.h"
#include "bam_index_host.h"
#include "bam_merge_host.h"
#include "bam_keys.h"
#include "bam_rec.h"
#include "zsource.h"
#include <rocprim/rocprim.hpp>
#include <fcntl.h>
#include <unistd.h>
#include <stdarg.h>
#include <algorithm>
#include <chrono>
#include <vector>

namespace {

constexpr int MAX_RUNS = 256;
constexpr uint64_t MIN_WINDOW = 65536, MAX_WINDOW = 1ull << 28;

struct RunTab {                                               // a run's unemitted records, as the round's kernels see them
  const uint64_t* key; const uint64_t* start; const uint64_t* addr; const uint32_t* len;
  uint64_t avail, delta, eoff, cnt;                           // delta: the window's data - the lowest window; eoff / cnt: the run's part of the round
};
static_assert(sizeof(RunTab) == 64, "RunTab");

__device__ __forceinline__ uint64_t lower_bound(const uint64_t* __restrict__ k, uint64_t n, uint64_t x) {   // the keys < x
  uint64_t lo = 0, hi = n;
  while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (k[mid] < x) lo = mid + 1; else hi = mid; }
  return lo;
}
__device__ __forceinline__ uint64_t upper_bound(const uint64_t* __restrict__ k, uint64_t n, uint64_t x) {   // the keys <= x
  uint64_t lo = 0, hi = n;
  while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (k[mid] <= x) lo = mid + 1; else hi = mid; }
  return lo;
}

// the first record whose key is smaller than the one in front of it (the last key of the window before in front of record 0)
__global__ void __launch_bounds__(256) mg_order(uint64_t n, const uint64_t* __restrict__ key, uint64_t before, unsigned long long* __restrict__ first_bad) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && key[i] < (i ? key[i - 1] : before)) atomicMin(first_bad, (unsigned long long)i);
}

// a lane per run: how many of its records the round emits, and their bytes
__global__ void __launch_bounds__(MAX_RUNS) mg_count(int k, const RunTab* __restrict__ tab, int has_bound, uint64_t bound_key, int bound_run,
                                                    uint64_t* __restrict__ out) {
  const int j = threadIdx.x;
  if (j >= k) return;
  const RunTab T = tab[j];
  uint64_t c = T.avail;
  if (has_bound && c) c = j <= bound_run ? upper_bound(T.key, T.avail, bound_key) : lower_bound(T.key, T.avail, bound_key);
  out[2 * j] = c;
  out[2 * j + 1] = c ? T.start[c] - T.start[0] : 0;
}

__global__ void __launch_bounds__(256) mg_rank(int k, const RunTab* __restrict__ tab, uint64_t E, uint32_t* __restrict__ slen, uint64_t* __restrict__ spos) {
  __shared__ RunTab T[MAX_RUNS];
  for (int j = threadIdx.x; j < k; j += blockDim.x) T[j] = tab[j];
  __syncthreads();
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= E) return;
  int lo = 0, hi = k - 1;                                     // the last run whose part starts at or in front of g (a run without records shares its start with the next)
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (T[mid].eoff <= g) lo = mid; else hi = mid - 1; }
  const int r = lo;
  const uint64_t i = g - T[r].eoff, x = T[r].key[i];
  uint64_t rank = i;
  for (int j = 0; j < r; j++) if (T[j].cnt) rank += upper_bound(T[j].key, T[j].cnt, x);
  for (int j = r + 1; j < k; j++) if (T[j].cnt) rank += lower_bound(T[j].key, T[j].cnt, x);
  if (rank < E) { slen[rank] = T[r].len[i]; spos[rank] = T[r].addr[i] + T[r].delta; }
}

// bam_sort.hip's index kernels over one round, in stream offsets: byte at[p] of the round is byte u0 + at[p] of the stream
struct MIdx {
  uint64_t n; Meta M; const uint64_t* at; uint64_t u0; int n_ref;
  int32_t c_ref; uint32_t c_bin;                              // the last record of the round before (c_ref = -1: none, or one without a coordinate)
  uint32_t* head; const uint64_t* hoff;
  uint64_t* rkey; uint64_t* rbeg; uint64_t* rend; unsigned long long* cont_end;
  unsigned long long* stat;                                   // per reference: first, last, n_mapped, n_unmapped, n_intv; behind them n_no_coor
  unsigned long long* lin; const uint64_t* lin_off;
};

__global__ void __launch_bounds__(256) mi_mark(MIdx A) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool nocoor = false;
  if (p < A.n) {
    const int32_t ref = A.M.ref[p];
    const uint32_t bf = A.M.binflag[p];
    const int32_t pref = p ? A.M.ref[p - 1] : A.c_ref;
    const uint32_t pbin = p ? (A.M.binflag[p - 1] & 0xffffu) : A.c_bin;
    nocoor = ref < 0;
    A.head[p] = (!nocoor && (pref != ref || pbin != (bf & 0xffffu))) ? 1u : 0u;
    if (!nocoor) {
      unsigned long long* S = A.stat + 5 * (uint64_t)ref;
      if (p == 0 || pref != ref) atomicMin(&S[0], (unsigned long long)(A.u0 + A.at[p]));
      if (p + 1 == A.n || A.M.ref[p + 1] != ref) atomicMax(&S[1], (unsigned long long)(A.u0 + A.at[p + 1]));
      atomicAdd(&S[(bf & 0x10000u) ? 3 : 2], 1ull);
    }
  }
  const unsigned long long m = __ballot(nocoor);
  if (m && (threadIdx.x & 63) == 0) atomicAdd(&A.stat[5 * (uint64_t)A.n_ref], (unsigned long long)__popcll(m));
}

__global__ void __launch_bounds__(256) mi_runs(MIdx A) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= A.n) return;
  const int32_t ref = A.M.ref[p];
  if (ref < 0) return;
  const uint64_t h = A.hoff[p + 1];                           // heads up to and with p; 0: p belongs to the chunk the round before left open
  if (A.head[p]) { A.rkey[h - 1] = ((uint64_t)(uint32_t)ref << 16) | (A.M.binflag[p] & 0xffffu); A.rbeg[h - 1] = A.u0 + A.at[p]; }
  if (p + 1 == A.n || A.head[p + 1] || A.M.ref[p + 1] < 0) {
    if (h) A.rend[h - 1] = A.u0 + A.at[p + 1]; else *A.cont_end = A.u0 + A.at[p + 1];
  }
}

__global__ void __launch_bounds__(256) mi_windows(MIdx A) {
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const int lane = threadIdx.x & 63;
  for (uint64_t p = wave; p < A.n; p += n_waves) {
    const int32_t ref = A.M.ref[p];
    if (ref < 0) continue;
    const uint64_t n_win = A.lin_off[ref + 1] - A.lin_off[ref];
    const uint64_t p0 = A.M.pos[p] < 0 ? 0 : (uint64_t)A.M.pos[p];
    const uint64_t w0 = min(p0 >> 14, n_win - 1), w1 = min((p0 + A.M.span[p] - 1) >> 14, n_win - 1);
    const unsigned long long ub = A.u0 + A.at[p];
    for (uint64_t w = w0 + lane; w <= w1; w += 64) atomicMin(&A.lin[A.lin_off[ref] + w], ub);
    if (lane == 0) atomicMax(&A.stat[5 * (uint64_t)ref + 4], (unsigned long long)(w1 + 1));
  }
}

inline size_t grown(size_t have, size_t want) { return want <= have ? 0 : std::max(want, (size_t)4096) - have; }   // what DevBuf::ensure adds, in items
// The merger's own arrays: DevBuf without its floor of 4096 items (two runs of a few records merge in the budget that sorted them), an eighth of slack
// so that windows of about one size do not allocate anew each time.  Contents are not kept.  Not bam_rec.h's Buf, whose slack has 16 items more: the
// budget arithmetic of grown() below counts by room().  (Timer, blocks_of, wave_blocks and wall_ms are bam_rec.h's.)
template <typename T> struct MergeBuf {
  T* p = nullptr; size_t n = 0;
  static size_t room(size_t want) { return want + want / 8; }
  bool ensure(size_t want) {
    if (want <= n) return true;
    if (p) (void)hipFree(p);
    p = nullptr; n = 0;
    if (hipMalloc((void**)&p, room(want) * sizeof(T)) != hipSuccess) return false;
    n = room(want);
    return true;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};
template <typename T> size_t grown(const MergeBuf<T>& b, size_t want) { return want <= b.n ? 0 : MergeBuf<T>::room(want) - b.n; }

struct Run {
  std::string path;
  int fd = -1;
  lra_bgzf_step z;
  uint64_t skip = 0, want = 0; off_t size = 0;                // header bytes still in front of the records; compressed bytes per refill; the file's size
  MergeBuf<uint64_t> start, key, addr; MergeBuf<uint32_t> ord, len;
  bool filled = false;
  uint64_t n = 0, e = 0;                                      // the window's whole records; how many of them are emitted
  uint64_t first = 0, used = 0;                               // the first record's offset in the window's data; the byte behind the last
  uint64_t rec_base = 0, before = 0, win_last = 0;            // records in front of the window; the last key in front of it; the window's last key
  size_t bytes() const {
    return z.d_comp.n + z.d_dec[0].n + z.d_dec[1].n + 8 * z.d_boff.n + 4 * z.d_bstat.n + 8 * (start.n + key.n + addr.n) + 4 * (ord.n + len.n);
  }
  void release() { z.release(); start.release(); key.release(); addr.release(); ord.release(); len.release(); if (fd >= 0) close(fd); fd = -1; }
};

typedef lra_merge_chunk Chunk;
typedef lra_merge_refs RefTable;

}  // namespace

struct lra_bam_merger {
  lra_ctx* ctx = nullptr;
  uint64_t max_bytes = 0, first = 0;
  std::vector<Run> runs;
  std::vector<uint8_t> header; RefTable refs; bool long_ref = false;
  std::vector<uint64_t> lin_off;
  // the round
  MergeBuf<uint8_t> small, pend, tail;                        // small: the runs' table (64 per run), the counts (16 per run), 16 words of results
  MergeBuf<uint64_t> at, spos, hoff, rkey, rbeg, rend; MergeBuf<uint32_t> slen, head, mspan, mbf; MergeBuf<int32_t> mref, mpos;
  MergeBuf<unsigned long long> stat, lin; MergeBuf<uint64_t> d_lin_off;
  MergeBuf<uint64_t> skey[2]; MergeBuf<uint32_t> sord[2]; MergeBuf<uint8_t> stemp;   // index: a reference's chunks by bin
  bool index_ready = false;
  uint64_t pend_len = 0, cursor = 0, cut = 0, u_total = 0;
  int32_t c_ref = -1; uint32_t c_bin = 0;
  std::vector<Chunk> chunks;
  std::vector<uint64_t> moff;
  std::vector<uint8_t> bai;
  bool finished = false, delivered = false;
  int failed = 0; std::string fail_msg;
  struct lra_bam_merger_stats S{};

  size_t dev_bytes() const {
    size_t b = small.n + pend.n + tail.n + 8 * (at.n + spos.n + hoff.n + rkey.n + rbeg.n + rend.n) + 4 * (slen.n + head.n + mspan.n + mbf.n + mref.n + mpos.n) +
               8 * (stat.n + lin.n + d_lin_off.n) + 8 * (skey[0].n + skey[1].n) + 4 * (sord[0].n + sord[1].n) + stemp.n;
    for (const Run& r : runs) b += r.bytes();
    return b;
  }
  void peak() { S.peak_device_bytes = std::max<uint64_t>(S.peak_device_bytes, dev_bytes()); }
  void release_round() {
    small.release(); pend.release(); tail.release(); at.release(); spos.release(); hoff.release(); rkey.release(); rbeg.release(); rend.release();
    slen.release(); head.release(); mspan.release(); mbf.release(); mref.release(); mpos.release();
  }
  void release_all() {
    for (Run& r : runs) r.release();
    release_round(); stat.release(); lin.release(); d_lin_off.release();
    skey[0].release(); skey[1].release(); sord[0].release(); sord[1].release(); stemp.release();
  }
  int fail(int code, const char* fmt, ...) __attribute__((format(printf, 3, 4))) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    failed = code; fail_msg = buf;
    (void)hipStreamSynchronize(ctx->stream);
    release_all();                                             // (a merger that failed only refuses: nothing stays on the device)
    return lra_set_err(ctx, code, "%s", buf);
  }
  // MergeBuf::ensure under the budget
  template <class T> int grab(MergeBuf<T>& b, size_t want, const char* what) {
    const size_t add = grown(b, want) * sizeof(T);
    if (add && dev_bytes() + add > max_bytes)
      return fail(LRA_ERR_NOMEM, "lra_bam_merger: %s needs %zu bytes of device memory, the budget is %llu", what, dev_bytes() + add, (unsigned long long)max_bytes);
    if (!b.ensure(want)) { (void)hipGetLastError(); return fail(LRA_ERR_NOMEM, "lra_bam_merger: hipMalloc of %zu bytes for %s failed", want * sizeof(T), what); }
    peak();
    return LRA_OK;
  }
  uint64_t round_members() const { return ctx->bgzf_round > 0 ? (uint64_t)ctx->bgzf_round : 2048; }
  RunTab* d_tab() { return (RunTab*)small.p; }
  uint64_t* d_cnt() { return (uint64_t*)(small.p + 64 * runs.size()); }
  uint64_t* d_misc() { return (uint64_t*)(small.p + 80 * runs.size()); }   // [0..3] the frame's result, [4..6] bs_keys' OR / AND / error count, [7] mg_order, [8] mi_runs' open end

  int refill(int r);
  int round();
  int index_round(uint64_t E, const uint64_t* d_at);
};

// The next window of run r: what the window before left behind its last whole record, then the whole members of the next `want` compressed bytes.
int lra_bam_merger::refill(int ri) {
  Run& R = runs[ri];
  hipStream_t st = ctx->stream;
  lra_bgzf_step& z = R.z;
  if (R.filled) { z.commit(R.used); S.refills[ri]++; }
  R.filled = true; R.n = R.e = 0;
  for (;;) {
    // the walk fill() will make, made first: the bytes it still holds and the next `want` of the file
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t held = z.comp_len - z.consumed, carry = z.dec_len - z.dec_used;
    const off_t fpos = z.file_eof ? 0 : lseek(R.fd, 0, SEEK_CUR);
    if (fpos < 0) return fail(LRA_ERR_INVALID, "lra_bam_merger: read of %s failed", R.path.c_str());
    const uint64_t rest = (uint64_t)std::max<off_t>(R.size - fpos, 0) + 1;   // (a refill that asks for a byte more than the file has sees its end)
    lra_bgzf_members m;
    for (;;) {
      R.want = std::min(R.want, rest);
      std::vector<uint8_t> look(held + (z.file_eof ? 0 : R.want));
      if (held) memcpy(look.data(), z.h_comp.p + z.consumed, held);
      uint64_t got = 0;
      bool eof = z.file_eof;
      if (!eof) {
        while (got < R.want) {
          const ssize_t k = pread(R.fd, look.data() + held + got, R.want - got, fpos + (off_t)got);
          if (k < 0) return fail(LRA_ERR_INVALID, "lra_bam_merger: read of %s failed", R.path.c_str());
          if (k == 0) break;
          got += (uint64_t)k;
        }
        eof = got < R.want;
      }
      m = lra_bgzf_walk(look.data(), held + got, eof, carry);
      if (!m.starved) break;
      R.want = std::max(R.want, held + got) * 2;
    }
    const uint64_t nb = m.in_off.size() - 1, D = m.out_off.back(), cap = D / 36 + 1;
    const int dst = z.cur ^ 1;
    const size_t add = grown(z.d_comp.n, m.p + 1) + grown(z.d_dec[dst].n, padded_tiles(D) + 64) + 8 * grown(z.d_boff.n, 2 * (nb + 1)) + 4 * grown(z.d_bstat.n, nb + 1) +
                       8 * grown(R.start, cap + 1);
    if (dev_bytes() + add > max_bytes)
      return fail(LRA_ERR_NOMEM, "lra_bam_merger: a window of %llu compressed bytes of %s (%llu bytes of records) needs %zu bytes of device memory, the budget is %llu",
                  (unsigned long long)m.p, R.path.c_str(), (unsigned long long)D, dev_bytes() + add, (unsigned long long)max_bytes);
    uint64_t want = R.want;
    const int rc = z.fill(ctx, R.fd, &want, lra_bgzf_launch_inflate_lut, "merge_h2d", "merge_inflate");
    if (rc == LRA_ERR_NOMEM) return fail(rc, "lra_bam_merger: %s failed for a window of %s", z.nomem_pinned ? "hipHostMalloc" : "hipMalloc", R.path.c_str());
    if (rc == LRA_ERR_INVALID) return fail(rc, "lra_bam_merger: read of %s failed", R.path.c_str());
    if (rc) return rc;
    S.ms_read_inflate += wall_ms(t0);
    if (int g = grab(R.start, cap + 1, "a window's record starts")) return g;
    peak();
    if (!z.err.empty()) return fail(LRA_ERR_INVALID, "lra_bam_merger: %s: %s", R.path.c_str(), z.err.c_str());
    const uint64_t dlen = z.dlen, start = std::min(R.skip, dlen);
    if (dlen == start && !z.at_end) { z.commit(dlen); R.skip -= start; continue; }   // the header alone
    uint64_t fr[4] = {0, start, 0, 0};
    uint64_t* misc = d_misc();
    Timer T(st);
    if (dlen > start) {
      lra_bam_launch_frame(st, z.data, start, dlen, R.start.p, cap, misc);
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(fr, misc, 32, hipMemcpyDeviceToHost, st));
      LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    const uint64_t n = fr[0];
    if (fr[2]) return fail(LRA_ERR_INVALID, "lra_bam_merger: %s: record %llu is a bad record (block_size %llu)", R.path.c_str(), (unsigned long long)(R.rec_base + n), (unsigned long long)fr[3]);
    if (z.at_end && fr[1] < dlen) return fail(LRA_ERR_INVALID, "lra_bam_merger: %s: record %llu is cut by the end of the file", R.path.c_str(), (unsigned long long)(R.rec_base + n));
    if (n == 0 && !z.at_end) { R.want = std::max(R.want, z.comp_len) * 2; continue; }   // one record longer than the window: a larger one, under the same check
    R.skip = 0; R.first = start; R.used = fr[1]; R.n = n;
    if (n) {
      if (int g = grab(R.key, n, "a window's keys")) return g;
      if (int g = grab(R.addr, n, "a window's record addresses")) return g;
      if (int g = grab(R.ord, n, "a window's ordinals")) return g;
      if (int g = grab(R.len, n, "a window's record lengths")) return g;
      const unsigned long long init[4] = {0ull, ~0ull, 0ull, ~0ull};
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(misc + 4, init, sizeof init, hipMemcpyHostToDevice, st));
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(R.start.p + n, misc + 1, 8, hipMemcpyDeviceToDevice, st));
      KeyArgs A; A.data = z.data + start; A.start = R.start.p; A.n = n; A.ord0 = 0; A.delta = start; A.n_ref = refs.n_ref;
      A.key = R.key.p; A.ord = R.ord.p; A.addr = R.addr.p; A.len = R.len.p; A.red = (unsigned long long*)(misc + 4); A.err = (uint32_t*)(misc + 6);
      hipLaunchKernelGGL(bs_keys, dim3(blocks_of(n)), dim3(256), 0, st, A);
      hipLaunchKernelGGL(mg_order, dim3(blocks_of(n)), dim3(256), 0, st, n, (const uint64_t*)R.key.p, R.before, (unsigned long long*)(misc + 7));
      unsigned long long res[4] = {0, 0, 0, 0};
      LRA_HIP_CHECK(ctx, hipGetLastError());
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(res, misc + 4, sizeof res, hipMemcpyDeviceToHost, st));
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(&R.win_last, R.key.p + n - 1, 8, hipMemcpyDeviceToHost, st));
      S.ms_frame_keys += T.stop();
      LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
      if ((uint32_t)res[2])
        return fail(LRA_ERR_INVALID, "lra_bam_merger: %s: a record among records %llu .. %llu is shorter than its fields say, or names a reference outside [-1, %d)",
                    R.path.c_str(), (unsigned long long)R.rec_base, (unsigned long long)(R.rec_base + n - 1), refs.n_ref);
      if (res[3] != ~0ull)
        return fail(LRA_ERR_INVALID, "lra_bam_merger: %s: record %llu sorts in front of the record before it: the file is not sorted by coordinate", R.path.c_str(),
                    (unsigned long long)(R.rec_base + res[3]));
      R.before = R.win_last;
      R.rec_base += n;
    } else S.ms_frame_keys += T.stop();
    if (z.at_end) {                                            // the file is wholly in its window: the step's staging buffers and its other half go back
      z.d_comp.release(); z.d_boff.release(); z.d_bstat.release(); z.d_dec[z.cur].release(); z.h_comp.release();
    }
    return LRA_OK;
  }
}

// the index's part of a round of E gathered records (their fields are in mref .. mbf)
int lra_bam_merger::index_round(uint64_t E, const uint64_t* d_at) {
  hipStream_t st = ctx->stream;
  const int n_ref = refs.n_ref;
  const size_t nStat = 5 * (size_t)n_ref + 1;
  if (!index_ready) {
    const uint64_t nW = lin_off[n_ref];
    if (int g = grab(stat, nStat, "the index's counters")) return g;
    if (int g = grab(d_lin_off, (size_t)n_ref + 1, "the index's window table")) return g;
    if (int g = grab(lin, nW + 1, "the linear index's windows")) return g;
    std::vector<unsigned long long> s0(nStat, 0);
    for (int r = 0; r < n_ref; r++) s0[5 * (size_t)r] = ~0ull;
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(stat.p, s0.data(), 8 * nStat, hipMemcpyHostToDevice, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(d_lin_off.p, lin_off.data(), 8 * ((size_t)n_ref + 1), hipMemcpyHostToDevice, st));
    LRA_HIP_CHECK(ctx, hipMemsetAsync(lin.p, 0xff, 8 * (nW + 1), st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));              // (s0 leaves scope)
    index_ready = true;
  }
  if (int g = grab(head, E, "the round's chunk heads")) return g;
  if (int g = grab(hoff, E + 1, "the round's chunk numbers")) return g;
  if (int g = grab(rkey, E, "the round's chunks")) return g;
  if (int g = grab(rbeg, E, "the round's chunks")) return g;
  if (int g = grab(rend, E, "the round's chunks")) return g;
  uint64_t* misc = d_misc();
  MIdx I;
  I.n = E; I.M = Meta{mref.p, mpos.p, mspan.p, mbf.p}; I.at = d_at; I.u0 = u_total; I.n_ref = n_ref; I.c_ref = c_ref; I.c_bin = c_bin;
  I.head = head.p; I.hoff = hoff.p; I.rkey = rkey.p; I.rbeg = rbeg.p; I.rend = rend.p; I.cont_end = (unsigned long long*)(misc + 8);
  I.stat = stat.p; I.lin = lin.p; I.lin_off = d_lin_off.p;
  Timer T(st);
  LRA_HIP_CHECK(ctx, hipMemsetAsync(misc + 8, 0xff, 8, st));
  hipLaunchKernelGGL(mi_mark, dim3(blocks_of(E)), dim3(256), 0, st, I);
  if (lra_exclusive_scan<uint32_t>(ctx, (long)E, head.p, hoff.p)) return fail(LRA_ERR_HIP, "lra_bam_merger: the scan of the chunk heads failed");
  hipLaunchKernelGGL(mi_runs, dim3(blocks_of(E)), dim3(256), 0, st, I);
  hipLaunchKernelGGL(mi_windows, dim3(wave_blocks(ctx, E)), dim3(256), 0, st, I);
  LRA_HIP_CHECK(ctx, hipGetLastError());
  uint64_t nc = 0, open_end = ~0ull; uint32_t last_bf = 0;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&nc, hoff.p + E, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&open_end, misc + 8, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&c_ref, mref.p + E - 1, 4, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&last_bf, mbf.p + E - 1, 4, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  c_bin = last_bf & 0xffffu;
  if (c_ref < 0) c_ref = -1;
  std::vector<uint64_t> k(nc), b(nc), e(nc);
  if (nc) {
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(k.data(), rkey.p, 8 * nc, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(b.data(), rbeg.p, 8 * nc, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(e.data(), rend.p, 8 * nc, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  }
  lra_merge_add_round(chunks, open_end, k.data(), b.data(), e.data(), nc);   // (a chunk that ran over the round's edge goes on)
  S.ms_index += T.stop();
  return LRA_OK;
}

// One round: refill the emptied windows, find the bound, count, rank, gather behind the pending bytes.  finished = true when no run has a record left.
int lra_bam_merger::round() {
  hipStream_t st = ctx->stream;
  const int k = (int)runs.size();
  if (int g = grab(small, 80 * (size_t)k + 128, "the runs' table")) return g;
  for (int r = 0; r < k; r++) {
    Run& R = runs[r];
    while (!R.filled || (R.e == R.n && !R.z.at_end)) if (int rc = refill(r)) return rc;
  }
  bool any = false, has_bound = false;
  uint64_t bound_key = 0; int bound_run = 0;
  for (int r = 0; r < k; r++) {
    const Run& R = runs[r];
    if (R.e < R.n) any = true;
    if (R.e < R.n && !R.z.at_end && (!has_bound || R.win_last < bound_key)) { has_bound = true; bound_key = R.win_last; bound_run = r; }   // (the lowest run of equal keys)
  }
  if (!any) { finished = true; return LRA_OK; }
  std::vector<RunTab> tab((size_t)k);
  const uint8_t* base = nullptr;
  for (int r = 0; r < k; r++) if (runs[r].e < runs[r].n && (!base || runs[r].z.data < base)) base = runs[r].z.data;
  for (int r = 0; r < k; r++) {
    const Run& R = runs[r];
    RunTab& T = tab[r];
    memset(&T, 0, sizeof T);
    T.avail = R.n - R.e;
    if (!T.avail) continue;
    T.key = R.key.p + R.e; T.start = R.start.p + R.e; T.addr = R.addr.p + R.e; T.len = R.len.p + R.e; T.delta = (uint64_t)(R.z.data - base);
  }
  std::vector<uint64_t> cnt(2 * (size_t)k);
  double ms_rank = 0;
  {
    Timer T(st);
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(d_tab(), tab.data(), sizeof(RunTab) * k, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(mg_count, dim3(1), dim3(MAX_RUNS), 0, st, k, (const RunTab*)d_tab(), has_bound ? 1 : 0, bound_key, bound_run, d_cnt());
    LRA_HIP_CHECK(ctx, hipGetLastError());
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(cnt.data(), d_cnt(), 16 * (size_t)k, hipMemcpyDeviceToHost, st));
    ms_rank += T.stop();
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  }
  uint64_t E = 0, B = 0;
  for (int r = 0; r < k; r++) { tab[r].eoff = E; tab[r].cnt = cnt[2 * r]; E += cnt[2 * r]; B += cnt[2 * r + 1]; }
  if (!E) return fail(LRA_ERR_INVALID, "lra_bam_merger: a round without records");   // (the bound's run emits its window: not reached)
  // the bytes the last round left go to the front of the round's buffer
  const uint64_t left = pend_len - cursor;
  if (left) if (int g = grab(tail, left, "the pending bytes")) return g;
  if (left) LRA_HIP_CHECK(ctx, hipMemcpyAsync(tail.p, pend.p + cursor, left, hipMemcpyDeviceToDevice, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  if (int g = grab(pend, left + B + 64, "a round's records behind the pending bytes")) return g;
  if (left) LRA_HIP_CHECK(ctx, hipMemcpyAsync(pend.p, tail.p, left, hipMemcpyDeviceToDevice, st));
  if (int g = grab(at, E + 1, "the round's record offsets")) return g;
  if (int g = grab(slen, E, "the round's record lengths")) return g;
  if (int g = grab(spos, E, "the round's record addresses")) return g;
  if (int g = grab(mref, E, "the round's record fields")) return g;
  if (int g = grab(mpos, E, "the round's record fields")) return g;
  if (int g = grab(mspan, E, "the round's record fields")) return g;
  if (int g = grab(mbf, E, "the round's record fields")) return g;
  {
    Timer T(st);
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(d_tab(), tab.data(), sizeof(RunTab) * k, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(mg_rank, dim3(blocks_of(E)), dim3(256), 0, st, k, (const RunTab*)d_tab(), E, slen.p, spos.p);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    ms_rank += T.stop();
  }
  S.ms_bound_rank += ms_rank;
  uint8_t* dst = pend.p + left;
  {
    Timer T(st);
    if (lra_exclusive_scan<uint32_t>(ctx, (long)E, slen.p, at.p)) return fail(LRA_ERR_HIP, "lra_bam_merger: the scan of the record lengths failed");
    lra_pack_strings_launch(st, ctx->num_cu, E, (const char*)base, spos.p, at.p, (char*)dst, B);
    LRA_HIP_CHECK(ctx, hipMemsetAsync(dst + B, 0, 64, st));
    hipLaunchKernelGGL(bs_span, dim3(wave_blocks(ctx, E)), dim3(256), 0, st, E, (const uint8_t*)dst, (const uint64_t*)at.p, Meta{mref.p, mpos.p, mspan.p, mbf.p});
    LRA_HIP_CHECK(ctx, hipGetLastError());
    S.ms_gather_span += T.stop();
  }
  if (!long_ref) if (int rc = index_round(E, at.p)) return rc;
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  for (int r = 0; r < k; r++) {
    Run& R = runs[r];
    R.e += tab[r].cnt;
    if (tab[r].cnt && R.e == R.n && R.z.at_end) R.release();   // the run is through
  }
  u_total += B;
  pend_len = left + B; cursor = 0; cut = pend_len / LRA_DFL_IN_MAX * LRA_DFL_IN_MAX;
  S.rounds++; S.records += E; S.bytes += B;
  return LRA_OK;
}

extern "C" int lra_bam_merger_create(lra_ctx* ctx, uint64_t max_bytes, uint64_t window_bytes, int n_runs, const char* const* paths,
                                     uint64_t first_member_file_offset, lra_bam_merger** out) {
  if (!ctx || !out || !max_bytes) return LRA_ERR_INVALID;
  *out = nullptr;
  if (n_runs < 1 || n_runs > MAX_RUNS) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_bam_merger_create: %d runs; one merger takes 1 .. %d files", n_runs, MAX_RUNS);
  if (!paths) return LRA_ERR_INVALID;
  std::unique_ptr<lra_bam_merger> m(new lra_bam_merger());
  m->ctx = ctx; m->max_bytes = max_bytes; m->first = first_member_file_offset;
  m->runs.resize((size_t)n_runs);
  const uint64_t window = window_bytes ? std::max(window_bytes, MIN_WINDOW) : std::min(std::max(max_bytes / (24 * (uint64_t)n_runs), MIN_WINDOW), MAX_WINDOW);
  for (int r = 0; r < n_runs; r++) {
    if (!paths[r]) return LRA_ERR_INVALID;
    Run& R = m->runs[r];
    R.path = paths[r]; R.want = window;
    uint64_t hdr = 0;
    if (lra_hts_sniff(R.path, &hdr) != LRA_IN_BAM) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_bam_merger_create: %s is not a BAM file", R.path.c_str());
    std::vector<uint8_t> h; std::string why; RefTable T;
    if (!lra_bam_read_header(R.path, hdr, h, why)) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_bam_merger_create: %s: %s", R.path.c_str(), why.c_str());
    if (!lra_merge_parse_refs(h.data(), h.size(), T)) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_bam_merger_create: %s: not a valid BAM header", R.path.c_str());
    R.skip = hdr;
    if (r == 0) { m->header.swap(h); m->refs = T; continue; }
    const RefTable& F = m->refs;
    const char* p0 = m->runs[0].path.c_str();
    if (T.n_ref != F.n_ref) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_bam_merger_create: %s has %d references, %s has %d", R.path.c_str(), T.n_ref, p0, F.n_ref);
    for (int32_t i = 0; i < T.n_ref; i++) {
      if (T.name[i] != F.name[i])
        return lra_set_err(ctx, LRA_ERR_INVALID, "lra_bam_merger_create: %s: reference %d is named %s, in %s it is %s", R.path.c_str(), i, T.name[i].c_str(), p0, F.name[i].c_str());
      if (T.len[i] != F.len[i])
        return lra_set_err(ctx, LRA_ERR_INVALID, "lra_bam_merger_create: %s: reference %d (%s) has length %llu, in %s it has %llu", R.path.c_str(), i, T.name[i].c_str(),
                           (unsigned long long)T.len[i], p0, (unsigned long long)F.len[i]);
    }
  }
  const int n_ref = m->refs.n_ref;
  m->lin_off.assign((size_t)n_ref + 1, 0);
  for (int r = 0; r < n_ref; r++) {
    if (m->refs.len[r] > LRA_BAI_MAX_REF) m->long_ref = true;
    m->lin_off[(size_t)r + 1] = m->lin_off[r] + lra_bai_windows(m->refs.len[r]);
  }
  // what stands whatever the windows hold: the tables, the pending bytes' buffer, the resident index
  const size_t fixed = 80 * (size_t)n_runs + 128 + (m->long_ref ? 0 : 8 * (5 * (size_t)n_ref + 1 + (size_t)n_ref + 1 + m->lin_off[n_ref] + 1));
  if (fixed > max_bytes)
    return lra_set_err(ctx, LRA_ERR_NOMEM, "lra_bam_merger_create: the tables and the index of %d references need %zu bytes of device memory, the budget is %llu", n_ref, fixed,
                       (unsigned long long)max_bytes);
  for (Run& R : m->runs) {
    R.fd = open(R.path.c_str(), O_RDONLY);
    R.size = R.fd < 0 ? 0 : lseek(R.fd, 0, SEEK_END);
    if (R.fd >= 0 && (R.size < 0 || lseek(R.fd, 0, SEEK_SET) != 0)) { close(R.fd); R.fd = -1; }
    if (R.fd < 0) { for (Run& Q : m->runs) Q.release(); return lra_set_err(ctx, LRA_ERR_INVALID, "lra_bam_merger_create: cannot open %s", R.path.c_str()); }
  }
  m->moff.assign(1, 0);
  *out = m.release();
  return LRA_OK;
}

extern "C" void lra_bam_merger_destroy(lra_bam_merger* m) {
  if (!m) return;
  (void)hipSetDevice(m->ctx->device);
  (void)hipStreamSynchronize(m->ctx->stream);
  m->release_all();
  delete m;
}

extern "C" int lra_bam_merger_header(lra_bam_merger* m, const uint8_t** h_bytes, uint64_t* len, int* n_ref, const uint64_t** ref_len) {
  if (!m) return LRA_ERR_INVALID;
  if (h_bytes) *h_bytes = m->header.data();
  if (len) *len = m->header.size();
  if (n_ref) *n_ref = m->refs.n_ref;
  if (ref_len) *ref_len = m->refs.len.data();
  return LRA_OK;
}

extern "C" int lra_bam_merger_stats(lra_bam_merger* m, struct lra_bam_merger_stats* out) {
  if (!m || !out) return LRA_ERR_INVALID;
  *out = m->S;
  return LRA_OK;
}

extern "C" int lra_bam_merger_next(lra_bam_merger* m, const uint8_t** h_data, uint64_t* len) {
  if (!m || !h_data || !len) return LRA_ERR_INVALID;
  lra_ctx* ctx = m->ctx;
  *h_data = nullptr; *len = 0;
  if (m->failed) return lra_set_err(ctx, m->failed, "%s", m->fail_msg.c_str());
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  for (;;) {
    if (m->cursor < m->cut) {
      const uint64_t slice = std::min<uint64_t>(m->cut - m->cursor, m->round_members() * (uint64_t)LRA_DFL_IN_MAX);
      const uint64_t* mo = nullptr; uint64_t nm = 0;
      const auto t0 = std::chrono::steady_clock::now();
      if (int rc = lra_bgzf_compress_device(ctx, m->pend.p + m->cursor, slice, h_data, len, &mo, &nm)) return rc;
      m->S.ms_compress += wall_ms(t0);
      const uint64_t base = m->moff.back();
      for (uint64_t i = 1; i <= nm; i++) m->moff.push_back(base + mo[i]);
      m->cursor += slice;
      return LRA_OK;
    }
    if (m->finished) {
      if (m->pend_len > m->cursor) { m->cut = m->pend_len; continue; }   // the last bytes: a member shorter than the others
      m->delivered = true;
      return LRA_OK;
    }
    if (int rc = m->round()) return rc;
  }
}

extern "C" int lra_bam_merger_index(lra_bam_merger* m, const uint8_t** h_bai, uint64_t* len) {
  if (!m || !h_bai || !len) return LRA_ERR_INVALID;
  lra_ctx* ctx = m->ctx;
  *h_bai = nullptr; *len = 0;
  if (m->failed) return lra_set_err(ctx, m->failed, "%s", m->fail_msg.c_str());
  if (!m->delivered) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_bam_merger_index: the last piece has not been taken");
  if (m->long_ref) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_bam_merger_index: a reference is longer than 2^29 bases, which a .bai index cannot address");
  if (!m->bai.empty()) { *h_bai = m->bai.data(); *len = m->bai.size(); return LRA_OK; }
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  for (Run& R : m->runs) R.release();                          // the windows are done with: their memory serves the chunks' sort
  m->release_round();
  const int n_ref = m->refs.n_ref;
  const size_t nStat = 5 * (size_t)n_ref + 1;
  const uint64_t nW = m->lin_off[n_ref];
  lra_bai_arrays A;
  std::vector<uint64_t> lin(nW, LRA_BAI_NONE);
  std::vector<unsigned long long> stat(nStat, 0);
  for (int r = 0; r < n_ref; r++) stat[5 * (size_t)r] = ~0ull;
  Timer T(st);
  if (m->index_ready) {
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(stat.data(), m->stat.p, 8 * nStat, hipMemcpyDeviceToHost, st));
    if (nW) LRA_HIP_CHECK(ctx, hipMemcpyAsync(lin.data(), m->lin.p, 8 * nW, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  }
  // a reference's chunks are contiguous in file order: stable by bin, one reference at a time
  const std::vector<Chunk>& C = m->chunks;
  std::vector<uint32_t> order(C.size());
  std::vector<uint64_t> hk; std::vector<uint32_t> ho;
  for (size_t a = 0; a < C.size();) {
    size_t b = a;
    while (b < C.size() && (C[b].key >> 16) == (C[a].key >> 16)) b++;
    const size_t nr = b - a;
    ho.resize(nr);
    for (size_t i = 0; i < nr; i++) ho[i] = (uint32_t)i;
    if (nr > 1) {
      hk.resize(nr);
      for (size_t i = 0; i < nr; i++) hk[i] = C[a + i].key & 0xffffu;
      size_t tb = 0;
      rocprim::double_buffer<uint64_t> K0(nullptr, nullptr);
      rocprim::double_buffer<uint32_t> V0(nullptr, nullptr);
      if (rocprim::radix_sort_pairs(nullptr, tb, K0, V0, nr, 0u, 16u, st) != hipSuccess) return m->fail(LRA_ERR_HIP, "lra_bam_merger_index: rocprim::radix_sort_pairs");
      for (int s = 0; s < 2; s++) {
        if (int g = m->grab(m->skey[s], nr, "the sort of a reference's chunks")) return g;
        if (int g = m->grab(m->sord[s], nr, "the sort of a reference's chunks")) return g;
      }
      if (int g = m->grab(m->stemp, tb + 1, "the sort of a reference's chunks")) return g;
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(m->skey[0].p, hk.data(), 8 * nr, hipMemcpyHostToDevice, st));
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(m->sord[0].p, ho.data(), 4 * nr, hipMemcpyHostToDevice, st));
      rocprim::double_buffer<uint64_t> K(m->skey[0].p, m->skey[1].p);
      rocprim::double_buffer<uint32_t> V(m->sord[0].p, m->sord[1].p);
      if (rocprim::radix_sort_pairs(m->stemp.p, tb, K, V, nr, 0u, 16u, st) != hipSuccess) return m->fail(LRA_ERR_HIP, "lra_bam_merger_index: rocprim::radix_sort_pairs");
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(ho.data(), V.current(), 4 * nr, hipMemcpyDeviceToHost, st));
      LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    for (size_t i = 0; i < nr; i++) order[a + i] = (uint32_t)(a + ho[i]);
    a = b;
  }
  m->S.ms_index += T.stop();
  lra_merge_index_arrays(C, order, stat.data(), std::move(lin), m->lin_off, m->moff.data(), m->first, A);
  lra_bai_write(A, m->bai);
  m->release_all();
  *h_bai = m->bai.data(); *len = m->bai.size();
  return LRA_OK;
}

// lra_amd/csrc/bam_sort.hip -- lra_bam_sorter: the raw BAM records of any number of batches, held in device memory of the sorter's own, sorted by coordinate
// and given back as BGZF members with the bytes of the .bai index (gfx950).  include/lra_hip.h has the interface, the order, the budget and the index's rules.
//
// finish.  bs_keys, a lane per held record: the core fields by bytes (a record starts at any alignment) -> the 64-bit key, the ordinal, the record's address
// and length; a wave reduction ORs and ANDs the keys, so rocprim's radix sort runs over the bits in which they differ only (a batch on three chromosomes
// without unmapped records sorts 35 bits, not 64).  The gather is the project's copy pass (lra_pack_strings_launch: the OUTPUT cut into 4 KiB chunks, a wave
// each) with src_pos = the address of record perm[p]: the batches' allocations are addressed from the lowest of them.  bs_span, a WAVE per sorted record: the
// lanes stride its CIGAR ops (aligned dwords, as wave_copy reads) and a wave reduction sums the ops that consume the reference -- a contig's 10^5 ops are
// 1600 steps of a wave, not one lane's walk.
// index.  bi_mark, a lane per record: run heads ((refID, bin) differs from the record in front), per reference the first / last offset and the mapped /
// unmapped counts, the records without a coordinate; a scan numbers the runs; bi_runs writes {ref << 16 | bin, vbeg, vend}; rocprim sorts the runs by the
// 47-bit key (stable: a bin's chunks stay in file order); bi_windows, a wave per record, 64-bit atomicMin of the record's start offset into the windows it
// touches, the lanes striding them; bi_fill, a wave per reference, the backward fill from the last touched window in tiles of 64.  The host counts the
// chunks of each bin while it writes the bytes (bam_index_host.h: one writer for the device's arrays and lra_bam_index_host's).
#include "common.h"
#include "chunk_copy.h"
#include "scan.h"
#include "bgzf_deflate.h"
#include "bam_index_host.h"
#include "bam_keys.h"
#include "bam_rec.h"
#include <rocprim/rocprim.hpp>
#include <chrono>
#include <vector>

namespace {

inline size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

struct Chunk { uint8_t* data; uint64_t* start; uint64_t n, bytes; size_t alloc; void* mem; };

// the sorted records' lengths and addresses: the gather's inputs
__global__ void __launch_bounds__(256) bs_permute(uint64_t n, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ len, const uint64_t* __restrict__ addr,
                                                 uint32_t* __restrict__ slen, uint64_t* __restrict__ spos) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n) { const uint32_t i = perm[p]; slen[p] = len[i]; spos[p] = addr[i]; }
}

struct IdxArgs {
  uint64_t n; Meta M; const uint64_t* at; const uint64_t* moff; uint64_t first; int n_ref;
  uint32_t* head; const uint64_t* hoff;
  uint64_t* runkey; uint32_t* runord; uint64_t* rbeg; uint64_t* rend;
  unsigned long long* stat;                                   // per reference: first, last, n_mapped, n_unmapped, n_intv; behind them n_no_coor
  unsigned long long* lin; const uint64_t* lin_off;
};
__device__ __forceinline__ uint64_t voff(const IdxArgs& A, uint64_t u) { return ((A.first + A.moff[u / LRA_DFL_IN_MAX]) << 16) | (u % LRA_DFL_IN_MAX); }

__global__ void __launch_bounds__(256) bi_mark(IdxArgs A) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool nocoor = false;
  if (p < A.n) {
    const int32_t ref = A.M.ref[p];
    const uint32_t bf = A.M.binflag[p];
    nocoor = ref < 0;
    A.head[p] = (!nocoor && (p == 0 || A.M.ref[p - 1] != ref || (A.M.binflag[p - 1] & 0xffffu) != (bf & 0xffffu))) ? 1u : 0u;
    if (!nocoor) {
      unsigned long long* S = A.stat + 5 * (uint64_t)ref;
      if (p == 0 || A.M.ref[p - 1] != ref) atomicMin(&S[0], (unsigned long long)voff(A, A.at[p]));
      if (p + 1 == A.n || A.M.ref[p + 1] != ref) atomicMax(&S[1], (unsigned long long)voff(A, A.at[p + 1]));
      atomicAdd(&S[(bf & 0x10000u) ? 3 : 2], 1ull);
    }
  }
  const unsigned long long m = __ballot(nocoor);
  if (m && (threadIdx.x & 63) == 0) atomicAdd(&A.stat[5 * (uint64_t)A.n_ref], (unsigned long long)__popcll(m));
}

__global__ void __launch_bounds__(256) bi_runs(IdxArgs A) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= A.n) return;
  const int32_t ref = A.M.ref[p];
  if (ref < 0) return;
  const uint64_t r = A.hoff[p + 1] - 1;                        // (heads up to and with p, less one: p's run)
  if (A.head[p]) { A.runkey[r] = ((uint64_t)(uint32_t)ref << 16) | (A.M.binflag[p] & 0xffffu); A.runord[r] = (uint32_t)r; A.rbeg[r] = voff(A, A.at[p]); }
  if (p + 1 == A.n || A.head[p + 1] || A.M.ref[p + 1] < 0) A.rend[r] = voff(A, A.at[p + 1]);
}

__global__ void __launch_bounds__(256) bi_windows(IdxArgs A) {
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const int lane = threadIdx.x & 63;
  for (uint64_t p = wave; p < A.n; p += n_waves) {
    const int32_t ref = A.M.ref[p];
    if (ref < 0) continue;
    const uint64_t n_win = A.lin_off[ref + 1] - A.lin_off[ref];
    const uint64_t p0 = A.M.pos[p] < 0 ? 0 : (uint64_t)A.M.pos[p];
    const uint64_t w0 = min(p0 >> 14, n_win - 1), w1 = min((p0 + A.M.span[p] - 1) >> 14, n_win - 1);
    const unsigned long long vb = voff(A, A.at[p]);
    for (uint64_t w = w0 + lane; w <= w1; w += 64) atomicMin(&A.lin[A.lin_off[ref] + w], vb);
    if (lane == 0) atomicMax(&A.stat[5 * (uint64_t)ref + 4], (unsigned long long)(w1 + 1));
  }
}

// a wave per reference: from the last touched window backward in tiles of 64, an untouched window takes the value of the next touched one behind it
__global__ void __launch_bounds__(64) bi_fill(IdxArgs A) {
  const int ref = blockIdx.x, lane = threadIdx.x;
  unsigned long long* L = A.lin + A.lin_off[ref];
  const uint64_t n = A.stat[5 * (uint64_t)ref + 4];
  unsigned long long carry = ~0ull;
  for (uint64_t hi = n; hi > 0; hi = hi > 64 ? hi - 64 : 0) {
    const uint64_t lo = hi > 64 ? hi - 64 : 0, w = lo + lane;
    unsigned long long x = w < hi ? L[w] : ~0ull;
    for (int d = 1; d < 64; d <<= 1) { const unsigned long long y = __shfl_down(x, d); if (lane + d < 64 && x == ~0ull) x = y; }
    if (x == ~0ull) x = carry;
    if (w < hi) L[w] = x;
    carry = __shfl(x, 0);
  }
}

size_t sort_temp(uint64_t n) {
  if (!n) return 0;
  size_t tb = 0;
  rocprim::double_buffer<uint64_t> k(nullptr, nullptr);
  rocprim::double_buffer<uint32_t> v(nullptr, nullptr);
  if (rocprim::radix_sort_pairs(nullptr, tb, k, v, (size_t)n, 0, 64, (hipStream_t)0) != hipSuccess) return (size_t)64 * n + (1u << 20);
  return tb;
}
inline uint64_t members_of(uint64_t bytes) { return (bytes + LRA_DFL_IN_MAX - 1) / LRA_DFL_IN_MAX; }
size_t keep_bytes(uint64_t N, uint64_t B) { return al(B + 64) + al(8 * (N + 1)) + 4 * al(4 * N); }
size_t sort_arena(uint64_t N) { return 2 * al(8 * N) + 2 * al(4 * N) + al(sort_temp(N)) + al(8 * N) + al(4 * N) + al(4 * N) + al(8 * N) + 256; }
size_t index_arena(uint64_t N, uint64_t B, size_t per_ref) {
  return al(4 * N) + al(8 * (N + 1)) + 2 * al(8 * N) + 2 * al(4 * N) + 2 * al(8 * N) + al(sort_temp(N)) + al(8 * (members_of(B) + 1)) + per_ref;
}
size_t round_bytes(uint64_t R) { return R ? 3 * al((R + 1) * 8) + 2 * al(R * 4) + 2 * (R * (size_t)LRA_DFL_SLOT + 256) : 0; }

}  // namespace

struct lra_bam_sorter {
  lra_ctx* ctx = nullptr;
  uint64_t max_bytes = 0;
  std::vector<Chunk> chunks;
  uint64_t n = 0, bytes = 0;                                  // held
  size_t held_alloc = 0;
  int state = 0;                                              // 0 collecting, 1 finished: the members are being delivered
  void* keep = nullptr;                                       // the sorted stream, its offsets, the per-record fields
  uint8_t* sorted = nullptr; uint64_t* at = nullptr; Meta M{};
  uint64_t cursor = 0, first = 0;
  int n_ref = 0; std::vector<uint64_t> ref_len; bool long_ref = false;
  std::vector<uint64_t> moff;
  std::vector<uint8_t> bai;
  double ms[5] = {0, 0, 0, 0, 0};
  void drop() {
    for (Chunk& c : chunks) (void)hipFree(c.mem);
    chunks.clear(); held_alloc = 0;
  }
  void reset() {
    drop();
    if (keep) (void)hipFree(keep);
    keep = nullptr; sorted = nullptr; at = nullptr; n = bytes = cursor = 0; state = 0; moff.clear();
  }
  uint64_t round() const { return ctx->bgzf_round > 0 ? (uint64_t)ctx->bgzf_round : 2048; }
  size_t need(uint64_t N, uint64_t B, size_t per_ref) const {
    return keep_bytes(N, B) + std::max(sort_arena(N), index_arena(N, B, per_ref)) + round_bytes(std::min(round(), members_of(B)));
  }
};

extern "C" int lra_bam_sorter_create(lra_ctx* ctx, uint64_t max_bytes, lra_bam_sorter** out) {
  if (!ctx || !out || !max_bytes) return LRA_ERR_INVALID;
  lra_bam_sorter* s = new lra_bam_sorter();
  s->ctx = ctx; s->max_bytes = max_bytes;
  *out = s;
  return LRA_OK;
}

extern "C" void lra_bam_sorter_destroy(lra_bam_sorter* s) {
  if (!s) return;
  (void)hipSetDevice(s->ctx->device);
  (void)hipStreamSynchronize(s->ctx->stream);
  s->reset();
  delete s;
}

extern "C" int lra_bam_sorter_held(lra_bam_sorter* s, uint64_t* n_rec, uint64_t* bytes) {
  if (!s) return LRA_ERR_INVALID;
  if (n_rec) *n_rec = s->n;
  if (bytes) *bytes = s->bytes;
  return LRA_OK;
}

extern "C" int lra_bam_sorter_stats(lra_bam_sorter* s, double ms[5]) {
  if (!s || !ms) return LRA_ERR_INVALID;
  for (int k = 0; k < 5; k++) ms[k] = s->ms[k];
  return LRA_OK;
}

extern "C" int lra_bam_sorter_add_device(lra_bam_sorter* s, const uint8_t* d_stream, const uint64_t* d_rec_start, uint64_t n_rec) {
  if (!s || (n_rec && (!d_stream || !d_rec_start))) return LRA_ERR_INVALID;
  lra_ctx* ctx = s->ctx;
  if (s->state != 0) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_bam_sorter_add_device: a finished run's members and index have not been taken");
  if (!n_rec) return LRA_OK;
  if (s->n + n_rec > 0xffffffffull) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_bam_sorter_add_device: more than 2^32 - 1 records held");
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  uint64_t ends[2] = {0, 0};
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&ends[0], d_rec_start, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&ends[1], d_rec_start + n_rec, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  if (ends[1] < ends[0]) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_bam_sorter_add_device: the record starts descend");
  const uint64_t B = ends[1] - ends[0];
  const size_t alloc = al(B + 64) + al(8 * (n_rec + 1));
  const size_t want = s->held_alloc + alloc + s->need(s->n + n_rec, s->bytes + B, 0);
  if (want > s->max_bytes)
    return lra_set_err(ctx, LRA_ERR_NOMEM, "lra_bam_sorter_add_device: %llu records of %llu bytes behind the %llu held need %zu bytes, the budget is %llu",
                       (unsigned long long)n_rec, (unsigned long long)B, (unsigned long long)s->n, want, (unsigned long long)s->max_bytes);
  void* mem = nullptr;
  if (hipMalloc(&mem, alloc) != hipSuccess) { (void)hipGetLastError(); return lra_set_err(ctx, LRA_ERR_NOMEM, "lra_bam_sorter_add_device: hipMalloc(%zu) failed", alloc); }
  Chunk c; c.mem = mem; c.data = (uint8_t*)mem; c.start = (uint64_t*)((char*)mem + al(B + 64)); c.n = n_rec; c.bytes = B; c.alloc = alloc;
  hipError_t e = B ? hipMemcpyAsync(c.data, d_stream + ends[0], B, hipMemcpyDeviceToDevice, st) : hipSuccess;
  if (e == hipSuccess) e = hipMemsetAsync(c.data + B, 0, 64, st);
  if (e == hipSuccess) e = hipMemcpyAsync(c.start, d_rec_start, 8 * (n_rec + 1), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) { (void)hipFree(mem); return lra_set_err(ctx, LRA_ERR_HIP, "lra_bam_sorter_add_device: %s", hipGetErrorString(e)); }
  s->chunks.push_back(c);
  s->n += n_rec; s->bytes += B; s->held_alloc += alloc;
  return LRA_OK;
}

extern "C" int lra_bam_sorter_finish(lra_bam_sorter* s, uint64_t first_member_file_offset, int n_ref, const uint64_t* ref_len) {
  if (!s || n_ref < 0 || (n_ref && !ref_len)) return LRA_ERR_INVALID;
  lra_ctx* ctx = s->ctx;
  if (s->state != 0) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_bam_sorter_finish: the run is finished already");
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const uint64_t N = s->n, B = s->bytes;
  bool long_ref = false;
  size_t per_ref = al(8 * (5 * (size_t)n_ref + 1)) + al(8 * ((size_t)n_ref + 1));
  for (int r = 0; r < n_ref; r++) { if (ref_len[r] > LRA_BAI_MAX_REF) long_ref = true; else per_ref += 8 * lra_bai_windows(ref_len[r]); }
  per_ref = al(per_ref);
  if (s->held_alloc + s->need(N, B, long_ref ? 0 : per_ref) > s->max_bytes)
    return lra_set_err(ctx, LRA_ERR_NOMEM, "lra_bam_sorter_finish: the index of %d references does not fit the budget of %llu bytes", n_ref, (unsigned long long)s->max_bytes);
  for (int k = 0; k < 5; k++) s->ms[k] = 0;
  if (N) {
    void* keep = nullptr; void* arena = nullptr;
    const size_t kb = keep_bytes(N, B), ab = sort_arena(N);
    if (hipMalloc(&keep, kb) != hipSuccess || hipMalloc(&arena, ab) != hipSuccess) {
      (void)hipGetLastError();
      if (keep) (void)hipFree(keep);
      return lra_set_err(ctx, LRA_ERR_NOMEM, "lra_bam_sorter_finish: hipMalloc(%zu + %zu) failed", kb, ab);
    }
    auto fail = [&](int code, const char* what) { (void)hipStreamSynchronize(st); (void)hipFree(keep); (void)hipFree(arena); return lra_set_err(ctx, code, "lra_bam_sorter_finish: %s", what); };
    char* w = (char*)keep;
    uint8_t* sorted = (uint8_t*)w; w += al(B + 64);
    uint64_t* at = (uint64_t*)w; w += al(8 * (N + 1));
    Meta M;
    M.ref = (int32_t*)w; w += al(4 * N); M.pos = (int32_t*)w; w += al(4 * N); M.span = (uint32_t*)w; w += al(4 * N); M.binflag = (uint32_t*)w;
    w = (char*)arena;
    uint64_t* key0 = (uint64_t*)w; w += al(8 * N);
    uint64_t* key1 = (uint64_t*)w; w += al(8 * N);
    uint32_t* ord0 = (uint32_t*)w; w += al(4 * N);
    uint32_t* ord1 = (uint32_t*)w; w += al(4 * N);
    size_t tb = sort_temp(N);
    void* temp = w; w += al(tb);
    uint64_t* addr = (uint64_t*)w; w += al(8 * N);
    uint32_t* len = (uint32_t*)w; w += al(4 * N);
    uint32_t* slen = (uint32_t*)w; w += al(4 * N);
    uint64_t* spos = (uint64_t*)w; w += al(8 * N);
    unsigned long long* red = (unsigned long long*)w;         // OR, AND, the error count
    const unsigned long long red0[3] = {0ull, ~0ull, 0ull};
    if (hipMemcpyAsync(red, red0, sizeof red0, hipMemcpyHostToDevice, st) != hipSuccess) return fail(LRA_ERR_HIP, "hipMemcpyAsync");
    const uint8_t* base = s->chunks[0].data;
    for (const Chunk& c : s->chunks) if (c.data < base) base = c.data;
    {
      Timer T(st);
      uint64_t o = 0;
      for (const Chunk& c : s->chunks) {
        KeyArgs A; A.data = c.data; A.start = c.start; A.n = c.n; A.ord0 = o; A.delta = (uint64_t)(c.data - base); A.n_ref = n_ref;
        A.key = key0; A.ord = ord0; A.addr = addr; A.len = len; A.red = red; A.err = (uint32_t*)(red + 2);
        hipLaunchKernelGGL(bs_keys, dim3(blocks_of(c.n)), dim3(256), 0, st, A);
        o += c.n;
      }
      s->ms[0] += T.stop();
    }
    unsigned long long h_red[3] = {0, 0, 0};
    if (hipMemcpyAsync(h_red, red, sizeof h_red, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess)
      return fail(LRA_ERR_HIP, "the key kernel failed");
    if ((uint32_t)h_red[2]) return fail(LRA_ERR_INVALID, "a held record is shorter than its fields say, or names a reference outside [-1, n_ref)");
    const unsigned long long differ = h_red[0] ^ h_red[1];
    const uint32_t* perm = ord0;
    if (differ) {
      const int begin_bit = __builtin_ctzll(differ), end_bit = 64 - __builtin_clzll(differ);
      Timer T(st);
      rocprim::double_buffer<uint64_t> K(key0, key1);
      rocprim::double_buffer<uint32_t> V(ord0, ord1);
      if (rocprim::radix_sort_pairs(temp, tb, K, V, (size_t)N, (unsigned)begin_bit, (unsigned)end_bit, st) != hipSuccess) return fail(LRA_ERR_HIP, "rocprim::radix_sort_pairs");
      perm = V.current();
      s->ms[1] = T.stop();
    }
    {
      Timer T(st);
      hipLaunchKernelGGL(bs_permute, dim3(blocks_of(N)), dim3(256), 0, st, N, perm, (const uint32_t*)len, (const uint64_t*)addr, slen, spos);
      if (lra_exclusive_scan<uint32_t>(ctx, (long)N, slen, at)) return fail(LRA_ERR_HIP, "the scan");
      lra_pack_strings_launch(st, ctx->num_cu, N, (const char*)base, spos, at, (char*)sorted, B);
      if (hipMemsetAsync(sorted + B, 0, 64, st) != hipSuccess) return fail(LRA_ERR_HIP, "hipMemsetAsync");
      s->ms[2] = T.stop();
    }
    {
      Timer T(st);
      hipLaunchKernelGGL(bs_span, dim3(wave_blocks(ctx, N)), dim3(256), 0, st, N, (const uint8_t*)sorted, (const uint64_t*)at, M);
      s->ms[0] += T.stop();
    }
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return fail(LRA_ERR_HIP, "a kernel of the sort failed");
    (void)hipFree(arena);
    s->keep = keep; s->sorted = sorted; s->at = at; s->M = M;
    s->drop();                                                 // (the sorted copy holds every record now)
  }
  s->first = first_member_file_offset; s->n_ref = n_ref; s->ref_len.assign(ref_len, ref_len + n_ref); s->long_ref = long_ref;
  s->cursor = 0; s->moff.assign(1, 0); s->state = 1;
  return LRA_OK;
}

extern "C" int lra_bam_sorter_next(lra_bam_sorter* s, const uint8_t** h_data, uint64_t* len) {
  if (!s || !h_data || !len) return LRA_ERR_INVALID;
  lra_ctx* ctx = s->ctx;
  *h_data = nullptr; *len = 0;
  if (s->state != 1) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_bam_sorter_next: no finished run");
  if (s->cursor >= s->bytes) return LRA_OK;
  const uint64_t slice = std::min<uint64_t>(s->bytes - s->cursor, s->round() * (uint64_t)LRA_DFL_IN_MAX);
  const uint64_t* mo = nullptr; uint64_t nm = 0;
  const auto t0 = std::chrono::steady_clock::now();
  if (int rc = lra_bgzf_compress_device(ctx, s->sorted + s->cursor, slice, h_data, len, &mo, &nm)) return rc;
  s->ms[3] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  const uint64_t base = s->moff.back();
  for (uint64_t i = 1; i <= nm; i++) s->moff.push_back(base + mo[i]);
  s->cursor += slice;
  return LRA_OK;
}

extern "C" int lra_bam_sorter_index(lra_bam_sorter* s, const uint8_t** h_bai, uint64_t* len) {
  if (!s || !h_bai || !len) return LRA_ERR_INVALID;
  lra_ctx* ctx = s->ctx;
  *h_bai = nullptr; *len = 0;
  if (s->state != 1 || s->cursor < s->bytes) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_bam_sorter_index: the run's last piece has not been taken");
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (s->long_ref) {
    s->reset();
    return lra_set_err(ctx, LRA_ERR_INVALID, "lra_bam_sorter_index: a reference is longer than 2^29 bases, which a .bai index cannot address");
  }
  const uint64_t N = s->n, B = s->bytes;
  const int n_ref = s->n_ref;
  lra_bai_arrays A;
  A.ref.resize((size_t)n_ref);
  A.lin_off.assign((size_t)n_ref + 1, 0);
  for (int r = 0; r < n_ref; r++) A.lin_off[(size_t)r + 1] = A.lin_off[r] + lra_bai_windows(s->ref_len[r]);
  const uint64_t nW = A.lin_off[n_ref], nM = s->moff.size() - 1;
  if (N) {
    const size_t tb = sort_temp(N), nStat = 5 * (size_t)n_ref + 1;
    const size_t ab = al(4 * N) + al(8 * (N + 1)) + 2 * al(8 * N) + 2 * al(4 * N) + 2 * al(8 * N) + al(tb) + al(8 * (nM + 1)) + al(8 * nStat) + al(8 * ((size_t)n_ref + 1)) + al(8 * nW);
    void* arena = nullptr;
    if (hipMalloc(&arena, ab) != hipSuccess) { (void)hipGetLastError(); return lra_set_err(ctx, LRA_ERR_NOMEM, "lra_bam_sorter_index: hipMalloc(%zu) failed", ab); }
    auto fail = [&](int code, const char* what) { (void)hipStreamSynchronize(st); (void)hipFree(arena); return lra_set_err(ctx, code, "lra_bam_sorter_index: %s", what); };
    char* w = (char*)arena;
    IdxArgs I; memset(&I, 0, sizeof I);
    I.n = N; I.M = s->M; I.at = s->at; I.first = s->first; I.n_ref = n_ref;
    I.head = (uint32_t*)w; w += al(4 * N);
    uint64_t* hoff = (uint64_t*)w; w += al(8 * (N + 1)); I.hoff = hoff;
    uint64_t* key0 = (uint64_t*)w; w += al(8 * N);
    uint64_t* key1 = (uint64_t*)w; w += al(8 * N);
    uint32_t* ord0 = (uint32_t*)w; w += al(4 * N);
    uint32_t* ord1 = (uint32_t*)w; w += al(4 * N);
    I.rbeg = (uint64_t*)w; w += al(8 * N);
    I.rend = (uint64_t*)w; w += al(8 * N);
    void* temp = w; w += al(tb);
    uint64_t* moff = (uint64_t*)w; w += al(8 * (nM + 1)); I.moff = moff;
    I.stat = (unsigned long long*)w; w += al(8 * nStat);
    uint64_t* lin_off = (uint64_t*)w; w += al(8 * ((size_t)n_ref + 1)); I.lin_off = lin_off;
    I.lin = (unsigned long long*)w;
    I.runkey = key0; I.runord = ord0;
    std::vector<unsigned long long> stat(nStat, 0);
    for (int r = 0; r < n_ref; r++) stat[5 * (size_t)r] = ~0ull;
    Timer T(st);
    if (hipMemcpyAsync(moff, s->moff.data(), 8 * (nM + 1), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(I.stat, stat.data(), 8 * nStat, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(lin_off, A.lin_off.data(), 8 * ((size_t)n_ref + 1), hipMemcpyHostToDevice, st) != hipSuccess ||
        (nW && hipMemsetAsync(I.lin, 0xff, 8 * nW, st) != hipSuccess))
      return fail(LRA_ERR_HIP, "the uploads failed");
    hipLaunchKernelGGL(bi_mark, dim3(blocks_of(N)), dim3(256), 0, st, I);
    if (lra_exclusive_scan<uint32_t>(ctx, (long)N, I.head, hoff)) return fail(LRA_ERR_HIP, "the scan");
    hipLaunchKernelGGL(bi_runs, dim3(blocks_of(N)), dim3(256), 0, st, I);
    hipLaunchKernelGGL(bi_windows, dim3(wave_blocks(ctx, N)), dim3(256), 0, st, I);
    if (n_ref) hipLaunchKernelGGL(bi_fill, dim3((unsigned)n_ref), dim3(64), 0, st, I);
    uint64_t nRuns = 0;
    if (hipMemcpyAsync(&nRuns, hoff + N, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return fail(LRA_ERR_HIP, "a kernel of the index failed");
    const uint64_t* skey = key0; const uint32_t* sord = ord0;
    if (nRuns > 1) {
      size_t tb2 = tb;
      rocprim::double_buffer<uint64_t> K(key0, key1);
      rocprim::double_buffer<uint32_t> V(ord0, ord1);
      if (rocprim::radix_sort_pairs(temp, tb2, K, V, (size_t)nRuns, 0u, 47u, st) != hipSuccess) return fail(LRA_ERR_HIP, "rocprim::radix_sort_pairs");
      skey = K.current(); sord = V.current();
    }
    std::vector<uint64_t> hk(nRuns), hb(nRuns), he(nRuns);
    std::vector<uint32_t> ho(nRuns);
    A.lin.resize(nW);
    hipError_t e = hipSuccess;
    if (nRuns) {
      e = hipMemcpyAsync(hk.data(), skey, 8 * nRuns, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipMemcpyAsync(ho.data(), sord, 4 * nRuns, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipMemcpyAsync(hb.data(), I.rbeg, 8 * nRuns, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipMemcpyAsync(he.data(), I.rend, 8 * nRuns, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(stat.data(), I.stat, 8 * nStat, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && nW) e = hipMemcpyAsync(A.lin.data(), I.lin, 8 * nW, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipGetLastError();
    s->ms[4] = T.stop();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(LRA_ERR_HIP, hipGetErrorString(e));
    (void)hipFree(arena);
    A.runs.resize(nRuns);
    for (uint64_t r = 0; r < nRuns; r++) A.runs[r] = lra_bai_run{(uint32_t)(hk[r] >> 16), (uint32_t)(hk[r] & 0xffffu), hb[ho[r]], he[ho[r]]};
    for (int r = 0; r < n_ref; r++) {
      lra_bai_ref& R = A.ref[r];
      R.first = stat[5 * (size_t)r]; R.last = stat[5 * (size_t)r + 1]; R.n_mapped = stat[5 * (size_t)r + 2]; R.n_unmapped = stat[5 * (size_t)r + 3]; R.n_intv = stat[5 * (size_t)r + 4];
    }
    A.n_no_coor = stat[nStat - 1];
  } else A.lin.assign(nW, LRA_BAI_NONE);
  (void)B;
  lra_bai_write(A, s->bai);
  s->reset();
  *h_bai = s->bai.data(); *len = s->bai.size();
  return LRA_OK;
}

extern "C" int lra_bam_index_host(const uint8_t* stream, uint64_t len, int n_ref, const uint64_t* ref_len, const uint64_t* member_off, uint64_t n_members,
                                  uint64_t first_member_file_offset, uint8_t* out, uint64_t cap, uint64_t* out_len) {
  return lra_bai_index(stream, len, n_ref, ref_len, member_off, n_members, first_member_file_offset, out, cap, out_len) ? LRA_ERR_INVALID : LRA_OK;
}

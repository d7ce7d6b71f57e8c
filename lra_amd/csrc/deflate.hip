// lra_amd/csrc/deflate.hip -- BGZF deflate (gfx950): lra_bgzf_deflate_batch / lra_bgzf_deflate_host, byte-identical members from bgzf_deflate.h's rules,
// and lra_bgzf_compress_device, the stream stage over a device text.
//
// bgzf_deflate: one wave (a workgroup of 64) per member.  LDS per wave: the hash table (4096 x 16 bit, 8 KB), a block's tokens (4096 x 32 bit, 16 KB),
// the block's tables (lra_dfl_tables, 4.6 KB), the output window (1 KB) and the CRC table (1 KB): 31 KB, five waves per CU.
//   parse    a group of 64 positions, a lane each: the candidate from the table as it stood, the match length, then the inserts -- every lane stores,
//            reads back and stores again while a lower position sits in its entry, so the highest position of a hash wins whatever order the stores
//            took (the value rises every round: at most as many rounds as lanes share the hash) --, then the greedy walk: a ballot of the lanes with a match, the walk jumps from match to match (the lanes between are literals).
//            The selected lanes' tokens go to LDS at the rank a popcount gives them; their symbols are counted with LDS atomic adds.
//   codes    lane 0 builds the block's codes (lra_dfl_build) and, for a dynamic block, writes its header into the output window with the serial writer.
//   bits     64 tokens at a time: a lane's token is at most 48 bits, a wave prefix sum over the lengths places them, the lanes OR them into the window
//            (LDS atomic or), and the window's complete dwords go to the slot: the member is written as whole dwords from its start, the header and
//            the trailer through the same path, the last one to three bytes singly.  A stored block's bytes take that path four to a lane.
//   CRC-32   a slice per lane over the member's data, combined as zlib's crc32_combine does (bgzf_inflate's way).
// What is read: the member's data bytes, nothing else.  What is written: [slot, slot + out_len), in dwords -- d_out must be 4-byte aligned.
#include "common.h"
#include "bgzf_deflate.h"
#include "chunk_copy.h"
#include "scan.h"
#include <algorithm>
#include <chrono>

namespace {

constexpr int DFL_HASH = 1 << LRA_DFL_HASH_BITS;
constexpr int DFL_WIN = 256;                                 // dwords of the output window: 31 bits left over + a dynamic header (< 4500 bits), or + 64 x 48 bits

// the host form's work arrays, kept over the members of a call
struct HostWork {
  std::vector<uint8_t> buf = std::vector<uint8_t>(LRA_DFL_SLOT + 1024, 0);   // the member's bits, ORed in: zero outside the last member's bytes
  std::vector<uint16_t> tab = std::vector<uint16_t>(DFL_HASH);
  std::vector<uint32_t> toks = std::vector<uint32_t>(LRA_DFL_BLOCK);
  uint32_t used = 0;                                                          // bytes of buf the last member wrote
};

void deflate_member_host(HostWork& W, const uint8_t* d, uint32_t n, uint8_t* slot, uint32_t* out_len) {
  std::vector<uint8_t>& buf = W.buf;
  std::vector<uint16_t>& tab = W.tab;
  std::vector<uint32_t>& toks = W.toks;
  std::fill(buf.begin(), buf.begin() + W.used, (uint8_t)0);
  std::fill(tab.begin(), tab.end(), (uint16_t)LRA_DFL_EMPTY);
  lra_dfl_tables t;
  uint64_t pos = 0;
  for (int i = 0; i < 18; i++) lra_dfl_put(buf.data(), &pos, lra_dfl_member_head(i), 8);
  uint32_t carry = 0;
  for (uint32_t b0 = 0;; b0 += LRA_DFL_BLOCK) {
    const uint32_t b1 = std::min(n, b0 + (uint32_t)LRA_DFL_BLOCK), rs = b0 + carry;
    uint32_t ntok = 0;
    memset(t.lfreq, 0, sizeof t.lfreq); memset(t.dfreq, 0, sizeof t.dfreq);
    for (uint32_t p0 = b0; p0 < b1; p0 += 64) {
      uint32_t mlen[64], dist[64];
      for (uint32_t l = 0; l < 64; l++) {                    // the candidates: the table as it stands at the group's start
        const uint32_t p = p0 + l;
        mlen[l] = 0; dist[l] = 0;
        if (p + 3 <= n) { const uint32_t cand = tab[lra_dfl_hash(d + p)]; mlen[l] = lra_dfl_match_len(d, n, p, cand); dist[l] = p - cand; }
      }
      for (uint32_t l = 0; l < 64; l++) if (p0 + l + 3 <= n) tab[lra_dfl_hash(d + p0 + l)] = (uint16_t)(p0 + l);   // ascending: the highest position wins
      uint32_t cur = carry;
      while (cur < 64 && p0 + cur < n) {
        uint32_t tok, ls, ds;
        if (mlen[cur]) { tok = lra_dfl_match_token(mlen[cur], dist[cur]); cur += mlen[cur]; } else { tok = d[p0 + cur]; cur++; }
        lra_dfl_token_syms(tok, &ls, &ds);
        t.lfreq[ls]++;
        if (ds != 0xffffffffu) t.dfreq[ds]++;
        toks[ntok++] = tok;
      }
      carry = cur > 64 ? cur - 64 : 0;
    }
    const uint32_t re = b1 == n ? n : b1 + carry;
    const int last = b1 >= n;
    t.lfreq[256]++;
    const uint32_t dyn = lra_dfl_build(t), sto = lra_dfl_stored_bits(pos, re - rs);
    if (dyn < sto) {
      lra_dfl_header(t, last, buf.data(), &pos);
      for (uint32_t i = 0; i <= ntok; i++) {
        uint32_t nb;
        const uint64_t v = lra_dfl_token_bits(t, i < ntok ? toks[i] : 256u, &nb);
        lra_dfl_put(buf.data(), &pos, (uint32_t)v, nb < 32 ? (int)nb : 32);
        if (nb > 32) lra_dfl_put(buf.data(), &pos, (uint32_t)(v >> 32), (int)nb - 32);
      }
    } else {
      const uint32_t L = re - rs;
      lra_dfl_put(buf.data(), &pos, (uint32_t)last, 3);
      lra_dfl_put(buf.data(), &pos, 0, (int)((0 - pos) & 7));
      lra_dfl_put(buf.data(), &pos, L | ((~L & 0xffffu) << 16), 32);
      for (uint32_t q = rs; q < re; q++) lra_dfl_put(buf.data(), &pos, d[q], 8);
    }
    if (last) break;
  }
  lra_dfl_put(buf.data(), &pos, 0, (int)((0 - pos) & 7));
  lra_dfl_put(buf.data(), &pos, lra_crc32_update(0, d, n, lra_crc32_table()), 32);
  lra_dfl_put(buf.data(), &pos, n, 32);
  const uint32_t total = (uint32_t)(pos >> 3);
  buf[16] = (uint8_t)((total - 1) & 255); buf[17] = (uint8_t)((total - 1) >> 8);
  memcpy(slot, buf.data(), total);
  W.used = total;
  *out_len = total;
}

// the output window of one wave: ob[0, DFL_WIN) in LDS holds the member's bits from dword `wbase` on, `rel` of them; fewer than 32 between two calls
struct BitOut { uint32_t* ob; uint32_t* g; uint32_t wbase, rel; };

// the window's complete dwords to the slot; the bits left over move to its front
__device__ __forceinline__ void win_flush(BitOut& o, int lane) {
  __syncthreads();
  const uint32_t nd = o.rel >> 5;
  for (uint32_t i = lane; i < nd; i += 64) if (o.wbase + i < LRA_DFL_SLOT / 4) o.g[o.wbase + i] = o.ob[i];
  const uint32_t part = o.ob[nd];
  __syncthreads();
  if (nd) for (uint32_t i = lane; i <= nd + 2 && i < (uint32_t)DFL_WIN; i += 64) o.ob[i] = i == 0 ? part : 0;
  __syncthreads();
  o.wbase += nd; o.rel &= 31;
}

// every lane's nb (0 .. 64) low bits of v (no bit set above them) behind each other in lane order
__device__ __forceinline__ void win_put(BitOut& o, uint64_t v, uint32_t nb, int lane) {
  uint32_t inc = nb;
  for (int d = 1; d < 64; d <<= 1) { const uint32_t x = (uint32_t)__shfl_up((int)inc, d); if (lane >= d) inc += x; }
  const uint32_t total = (uint32_t)__shfl((int)inc, 63);
  if (nb) {
    const uint32_t off = o.rel + inc - nb, w = off >> 5, sh = off & 31;
    const uint64_t lo = v << sh;
    const uint32_t hi = sh ? (uint32_t)(v >> (64 - sh)) : 0;
    atomicOr(&o.ob[w], (uint32_t)lo);
    if (lo >> 32) atomicOr(&o.ob[w + 1], (uint32_t)(lo >> 32));
    if (hi) atomicOr(&o.ob[w + 2], hi);
  }
  o.rel += total;
  win_flush(o, lane);
}

__global__ void __launch_bounds__(64) bgzf_deflate(int n_blocks, const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off, uint8_t* out,
                                                   uint32_t* __restrict__ out_len, int32_t* __restrict__ status) {
  __shared__ uint16_t tab[DFL_HASH];
  __shared__ uint32_t toks[LRA_DFL_BLOCK];
  __shared__ lra_dfl_tables t;
  __shared__ uint32_t ob[DFL_WIN];
  __shared__ uint32_t crc_tab[256];
  const int lane = threadIdx.x;
  const long b = blockIdx.x;
  if (b >= n_blocks) return;
  const uint64_t i0 = in_off[b], len64 = in_off[b + 1] - i0;
  if (len64 > LRA_DFL_IN_MAX) { if (lane == 0) { status[b] = LRA_BGZF_ERR_ISIZE; out_len[b] = 0; } return; }
  const uint32_t n = (uint32_t)len64;
  const uint8_t* d = in + i0;
  uint8_t* slot = out + (uint64_t)b * LRA_DFL_SLOT;
  for (int i = lane; i < 256; i += 64) { crc_tab[i] = lra_crc32_table_entry((uint32_t)i); ob[i] = 0; }
  for (int i = lane; i < DFL_HASH; i += 64) tab[i] = (uint16_t)LRA_DFL_EMPTY;
  __syncthreads();
  uint32_t crc = 0;
  {
    const uint32_t slice = (n + 63) / 64, lo = min(lane * slice, n), hi = min(lo + slice, n);
    if (hi > lo) crc = lra_crc32_shift(lra_crc32_update(0, d + lo, hi - lo, crc_tab), n - hi);
    for (int s = 32; s > 0; s >>= 1) crc ^= (uint32_t)__shfl_xor((int)crc, s);
  }
  BitOut o{ob, (uint32_t*)slot, 0, 0};
  win_put(o, lane < 18 ? lra_dfl_member_head(lane) : 0, lane < 18 ? 8 : 0, lane);
  uint32_t carry = 0;
  for (uint32_t b0 = 0;; b0 += LRA_DFL_BLOCK) {
    const uint32_t b1 = min(n, b0 + (uint32_t)LRA_DFL_BLOCK), rs = b0 + carry;
    uint32_t ntok = 0;
    for (int i = lane; i < 288; i += 64) t.lfreq[i] = 0;
    if (lane < 32) t.dfreq[lane] = 0;
    __syncthreads();
    for (uint32_t p0 = b0; p0 < b1; p0 += 64) {
      const uint32_t p = p0 + lane;
      const bool ins = p + 3 <= n;
      uint32_t h = 0, mlen = 0, dist = 0;
      if (ins) {
        h = lra_dfl_hash(d + p);
        const uint32_t cand = tab[h];
        mlen = lra_dfl_match_len(d, n, p, cand);
        dist = p - cand;
      }
      __syncthreads();                                       // every candidate is read before the first insert
      if (ins) tab[h] = (uint16_t)p;
      for (;;) {                                             // the highest position of a hash stays
        __syncthreads();
        const bool need = ins && (uint32_t)tab[h] < p;
        if (!__ballot(need)) break;
        if (need) tab[h] = (uint16_t)p;
      }
      const unsigned long long M = __ballot(mlen != 0);
      unsigned long long S = 0;
      uint32_t cur = carry;
      while (cur < 64) {
        const unsigned long long rest = M & (~0ull << cur);
        if (!rest) { S |= ~0ull << cur; cur = 64; break; }
        const uint32_t m = (uint32_t)__builtin_ctzll(rest);
        S |= (~0ull << cur) & (m == 63 ? ~0ull : ((1ull << (m + 1)) - 1));
        cur = m + (uint32_t)__shfl((int)mlen, (int)m);
      }
      carry = cur > 64 ? cur - 64 : 0;
      if (p0 + 64 > n) S &= (1ull << (n - p0)) - 1;          // (n - p0 < 64 here)
      if ((S >> lane) & 1) {
        const uint32_t tok = mlen ? lra_dfl_match_token(mlen, dist) : (uint32_t)d[p];
        uint32_t ls, ds;
        lra_dfl_token_syms(tok, &ls, &ds);
        toks[ntok + (uint32_t)__popcll(S & ((1ull << lane) - 1))] = tok;
        atomicAdd(&t.lfreq[ls], 1u);
        if (ds != 0xffffffffu) atomicAdd(&t.dfreq[ds], 1u);
      }
      ntok += (uint32_t)__popcll(S);
    }
    const uint32_t re = b1 == n ? n : b1 + carry;
    const int last = b1 >= n;
    __syncthreads();
    uint32_t dyn = 0;
    if (lane == 0) { t.lfreq[256]++; dyn = lra_dfl_build(t); }
    dyn = (uint32_t)__shfl((int)dyn, 0);
    __syncthreads();
    const uint64_t pos = (uint64_t)o.wbase * 32 + o.rel;
    if (dyn < lra_dfl_stored_bits(pos, re - rs)) {
      uint64_t hp = o.rel;
      if (lane == 0) lra_dfl_header(t, last, (uint8_t*)ob, &hp);
      o.rel = (uint32_t)__shfl((int)(uint32_t)hp, 0);
      win_flush(o, lane);
      for (uint32_t i0t = 0; i0t <= ntok; i0t += 64) {
        const uint32_t i = i0t + lane;
        uint32_t nb = 0;
        uint64_t v = 0;
        if (i <= ntok) v = lra_dfl_token_bits(t, i < ntok ? toks[i] : 256u, &nb);
        win_put(o, v, nb, lane);
      }
    } else {
      const uint32_t L = re - rs, pad = (uint32_t)((0 - (pos + 3)) & 7);
      const uint64_t v = (uint64_t)last | ((uint64_t)(L | ((~L & 0xffffu) << 16)) << (3 + pad));
      win_put(o, lane == 0 ? v : 0, lane == 0 ? 35 + pad : 0, lane);
      for (uint32_t q = rs; q < re; q += 256) {
        const uint32_t a = q + 4 * lane, cnt = a < re ? min(4u, re - a) : 0;
        uint64_t w = 0;
        for (uint32_t k = 0; k < cnt; k++) w |= (uint64_t)d[a + k] << (8 * k);
        win_put(o, w, 8 * cnt, lane);
      }
    }
    if (last) break;
  }
  win_put(o, 0, lane == 0 ? (uint32_t)((0 - o.rel) & 7) : 0, lane);
  win_put(o, (uint64_t)crc | ((uint64_t)n << 32), lane == 0 ? 64 : 0, lane);
  const uint32_t tail = o.rel >> 3, total = o.wbase * 4 + tail;
  if (lane < (int)tail) slot[o.wbase * 4 + lane] = (uint8_t)(ob[0] >> (8 * lane));
  __threadfence();
  __syncthreads();
  if (lane == 0) {
    slot[16] = (uint8_t)((total - 1) & 255); slot[17] = (uint8_t)((total - 1) >> 8);
    out_len[b] = total; status[b] = LRA_BGZF_OK;
  }
}

// a round's member table: member i of the round is text[min(len, (first + i) * IN_MAX), ...) and lies in slot i
__global__ void bgzf_round_table(uint64_t first, uint64_t nr, uint64_t len, uint64_t* __restrict__ in_off, uint64_t* __restrict__ slot_pos) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= nr) in_off[i] = min(len, (first + i) * (uint64_t)LRA_DFL_IN_MAX);
  if (i < nr) slot_pos[i] = i * (uint64_t)LRA_DFL_SLOT;
}

constexpr int ROUND_SLOT = 22, PACKED_SLOT = 23;
constexpr int ROUND_DEFAULT = 2048;                          // members per round: 128 MiB of slots and as much for the round's packed members

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" int lra_bgzf_deflate_batch(lra_ctx* ctx, int n_blocks, const uint8_t* d_in, const uint64_t* d_in_off, uint8_t* d_out, uint32_t* d_out_len,
                                      int32_t* d_status) {
  if (!ctx || n_blocks < 0 || (n_blocks && (!d_in_off || !d_out || !d_out_len || !d_status)) || ((uintptr_t)d_out & 3)) return LRA_ERR_INVALID;
  if (!n_blocks) return LRA_OK;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  lra_time_begin(ctx, "bgzf_deflate");
  hipLaunchKernelGGL(bgzf_deflate, dim3((unsigned)n_blocks), dim3(64), 0, ctx->stream, n_blocks, d_in, d_in_off, d_out, d_out_len, d_status);
  lra_time_end(ctx);
  LRA_HIP_CHECK(ctx, hipGetLastError());
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return LRA_OK;
}

extern "C" int lra_bgzf_deflate_host(int n_blocks, const uint8_t* in, const uint64_t* in_off, uint8_t* out, uint32_t* out_len, int32_t* status) {
  if (n_blocks < 0 || (n_blocks && (!in_off || !out || !out_len || !status))) return LRA_ERR_INVALID;
  HostWork W;
  for (int b = 0; b < n_blocks; b++) {
    const uint64_t len = in_off[b + 1] - in_off[b];
    if (len > LRA_DFL_IN_MAX) { status[b] = LRA_BGZF_ERR_ISIZE; out_len[b] = 0; continue; }
    deflate_member_host(W, in + in_off[b], (uint32_t)len, out + (uint64_t)b * LRA_DFL_SLOT, &out_len[b]);
    status[b] = LRA_BGZF_OK;
  }
  return LRA_OK;
}

extern "C" int lra_bgzf_compress_set_round(lra_ctx* ctx, int members) {
  if (!ctx || members < 0) return LRA_ERR_INVALID;
  ctx->bgzf_round = members;
  return LRA_OK;
}

extern "C" int lra_bgzf_compress_stats(lra_ctx* ctx, double* ms_deflate, uint64_t* bgzf_bytes) {
  if (!ctx) return LRA_ERR_INVALID;
  if (ms_deflate) *ms_deflate = ctx->bgzf_ms;
  if (bgzf_bytes) *bgzf_bytes = ctx->bgzf_bytes;
  return LRA_OK;
}

extern "C" int lra_bgzf_compress_device(lra_ctx* ctx, const uint8_t* d_text, uint64_t len, const uint8_t** h_data, uint64_t* data_len,
                                        const uint64_t** h_member_off, uint64_t* n_members) {
  if (!ctx || (len && !d_text)) return LRA_ERR_INVALID;
  const auto t0 = std::chrono::steady_clock::now();
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const uint64_t n = (len + LRA_DFL_IN_MAX - 1) / LRA_DFL_IN_MAX;
  std::vector<uint64_t>& moff = ctx->bgzf_member_off;
  moff.assign(1, 0);
  moff.reserve(n + 1);
  uint64_t base = 0;
  if (n) {
    const uint64_t R = std::min<uint64_t>(n, ctx->bgzf_round > 0 ? (uint64_t)ctx->bgzf_round : (uint64_t)ROUND_DEFAULT);
    char* w = (char*)lra_ensure(ctx, ROUND_SLOT, 3 * al256((R + 1) * 8) + 2 * al256(R * 4) + R * (size_t)LRA_DFL_SLOT + 256);
    uint8_t* packed = (uint8_t*)lra_ensure(ctx, PACKED_SLOT, R * (size_t)LRA_DFL_SLOT + 256);
    if (!w || !packed) return lra_set_err(ctx, LRA_ERR_NOMEM, "lra_bgzf_compress_device: no memory for a round of %llu members", (unsigned long long)R);
    uint64_t* in_off = (uint64_t*)w; w += al256((R + 1) * 8);
    uint64_t* slot_pos = (uint64_t*)w; w += al256((R + 1) * 8);
    uint64_t* off = (uint64_t*)w; w += al256((R + 1) * 8);
    uint32_t* mlen = (uint32_t*)w; w += al256(R * 4);
    int32_t* mst = (int32_t*)w; w += al256(R * 4);
    uint8_t* slots = (uint8_t*)w;
    std::vector<uint32_t> h_len(R);
    std::vector<int32_t> h_st(R);
    for (uint64_t first = 0; first < n; first += R) {
      const uint64_t nr = std::min(R, n - first);
      hipLaunchKernelGGL(bgzf_round_table, dim3((unsigned)((nr + 256) / 256)), dim3(256), 0, st, first, nr, len, in_off, slot_pos);
      lra_time_begin(ctx, "bgzf_deflate");
      hipLaunchKernelGGL(bgzf_deflate, dim3((unsigned)nr), dim3(64), 0, st, (int)nr, d_text, in_off, slots, mlen, mst);
      lra_time_end(ctx);
      if (int rc = lra_exclusive_scan<uint32_t>(ctx, (long)nr, mlen, off)) return rc;
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(h_len.data(), mlen, nr * 4, hipMemcpyDeviceToHost, st));
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(h_st.data(), mst, nr * 4, hipMemcpyDeviceToHost, st));
      LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
      uint64_t total = 0;
      for (uint64_t i = 0; i < nr; i++) {
        if (h_st[i]) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_bgzf_compress_device: member %llu has status %d", (unsigned long long)(first + i), h_st[i]);
        total += h_len[i];
        moff.push_back(base + total);
      }
      lra_time_begin(ctx, "bgzf_pack");
      lra_pack_strings_launch(st, ctx->num_cu, nr, (const char*)slots, slot_pos, off, (char*)packed, total);
      lra_time_end(ctx);
      LRA_HIP_CHECK(ctx, hipGetLastError());
      if (ctx->bgzf_pin_bytes < base + total) {              // the page-locked buffer: kept, grown to what the rounds so far promise for the whole text
        const size_t want = (size_t)((double)(base + total) * ((double)n / (double)(first + nr)) * 1.1) + 4096;
        void* np = nullptr;
        if (hipHostMalloc(&np, want, hipHostMallocDefault) != hipSuccess) return lra_set_err(ctx, LRA_ERR_NOMEM, "hipHostMalloc(%zu) failed", want);
        if (base) memcpy(np, ctx->bgzf_pin, base);
        if (ctx->bgzf_pin) (void)hipHostFree(ctx->bgzf_pin);
        ctx->bgzf_pin = np; ctx->bgzf_pin_bytes = want;
      }
      LRA_HIP_CHECK(ctx, hipMemcpyAsync((char*)ctx->bgzf_pin + base, packed, total, hipMemcpyDeviceToHost, st));
      LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
      base += total;
    }
  }
  ctx->bgzf_bytes = base;
  ctx->bgzf_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (h_data) *h_data = (const uint8_t*)ctx->bgzf_pin;
  if (data_len) *data_len = base;
  if (h_member_off) *h_member_off = moff.data();
  if (n_members) *n_members = n;
  return LRA_OK;
}

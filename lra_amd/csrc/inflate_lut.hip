// lra_amd/csrc/inflate_lut.hip -- bgzf_inflate_lut: BGZF inflate with lookup tables, the contract of input_bam.hip's bgzf_inflate (one member per wave,
// the same member tables, the same nine status codes of bgzf.h, CRC-32 and ISIZE checked).  Nothing is read outside in[in_off[i], in_off[i+1]) and nothing is
// written outside out[out_off[i], out_off[i+1]).
//
// bgzf_inflate decodes a bit per step in one lane and stores every output byte on its own.  Here the whole wave runs the decoder with wave-uniform state (the
// bit buffer, the positions and the table entries are made uniform with readfirstlane, so the symbol loop is scalar work) and the lanes share what is parallel:
//   tables   per wave in LDS: literal/length codes of up to 10 bits (2^10 entries) and distance codes of up to 8 bits (2^8 entries), 5 KiB.  An entry packs
//            the code length, the extra-bit count, the kind and the literal / base value; one peek of the bit buffer decodes a symbol.  A longer code (or a
//            pattern no code starts) has the escape entry 0: bgzf.h's canonical count / symbol walk (lra_infl_decode) decodes it from the same bit buffer, so
//            the statuses are those of the shared decoder.  Lane 0 reads a dynamic block's code lengths with bgzf.h's lra_infl_dynamic_tables (serial by
//            nature); then every lane decodes 16 + 4 of the table indices by that walk over the index's bits.  The fixed-code tables are built the same way
//            when a fixed block needs them and kept until a dynamic block replaces them.
//   input    each lane holds one aligned dword of a 256-byte block of the member (a dword the member's range cuts is put together from the bytes inside the
//            range); the 64-bit bit buffer is refilled from the lanes by readlane: one wait for memory per 256 bytes, not per refill.
//   output   a 4 KiB ring in LDS, laid out so that a dword of the ring is an aligned dword of `out`.  A literal is one LDS byte; a match is copied by the
//            lanes, byte k from the byte (k mod distance) of its source, which is what the serial copy gives for every overlap (down to distance 1) and
//            reads only bytes written before the match.  Sources no longer in the ring are read from `out`: they were written out before (see flush).  When
//            2 KiB are pending the wave writes them to `out` in whole dwords (bytes only at the member's two unaligned ends).
//   CRC-32   as bgzf_inflate: a slice per lane over the member's output, combined as zlib's crc32_combine does.
// Plain HIP: no inline assembly, no scalar memory writes.
#include "common.h"
#include "bam_kernels.h"
#include "bgzf.h"

namespace {

constexpr int WAVES = 4;
constexpr int LIT_BITS = 10, DIST_BITS = 8;
constexpr uint32_t RING = 4096, RING_MASK = RING - 1, PENDING = 2048;

// a table entry: bits 0-3 code length (0: escape), 4-7 extra bits, 8-9 kind, 16-31 the literal or the base value
enum { K_LIT = 0, K_END = 1, K_LEN = 2, K_BAD = 3 };
__device__ inline uint32_t lit_entry(int sym, int len) {
  if (sym < 256) return (uint32_t)len | (K_LIT << 8) | ((uint32_t)sym << 16);
  if (sym == 256) return (uint32_t)len | (K_END << 8);
  sym -= 257;
  if (sym >= 29) return (uint32_t)len | (K_BAD << 8);
  const int ext = sym < 8 || sym == 28 ? 0 : (sym - 4) >> 2;
  const int base = sym < 8 ? 3 + sym : sym == 28 ? 258 : ((4 + (sym & 3)) << ext) + 3;
  return (uint32_t)len | ((uint32_t)ext << 4) | (K_LEN << 8) | ((uint32_t)base << 16);
}
__device__ inline uint32_t dist_entry(int sym, int len) {
  if (sym >= 30) return (uint32_t)len | (K_BAD << 8);
  const int ext = sym < 4 ? 0 : (sym - 2) >> 1;
  const int base = sym < 4 ? 1 + sym : ((2 + (sym & 1)) << ext) + 1;
  return (uint32_t)len | ((uint32_t)ext << 4) | ((uint32_t)base << 16);
}

// the canonical walk of lra_infl_decode over the bits of a table index: the symbol whose code (of at most `bits` bits) the index starts with; -1: none
__device__ inline int walk_index(uint32_t idx, int bits, const int16_t* cnt, const int16_t* sym, int* len_out) {
  int code = 0, first = 0, index = 0;
  for (int len = 1; len <= bits; len++) {
    code |= (int)((idx >> (len - 1)) & 1u);
    const int count = cnt[len];
    if (code - count < first) { *len_out = len; return sym[index + (code - first)]; }
    index += count; first += count; first <<= 1; code <<= 1;
  }
  return -1;
}

struct WaveLds {
  uint32_t lit[1 << LIT_BITS], dist[1 << DIST_BITS];
  uint32_t ring[RING / 4];
  lra_inflate_tables t;
};

// the decoder's state: wave-uniform.  in / inlen / incnt / bitbuf / bitcnt / err are the fields bgzf.h's templates (lra_infl_bits, lra_infl_decode,
// lra_infl_dynamic_tables) work on, so the escape path and the block headers run the shared code on this state
struct State {
  const uint8_t* in; uint32_t inlen, incnt;
  uint64_t bitbuf; int bitcnt;
  int err;
};

__device__ inline uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ inline void make_uniform(State& s) {
  s.incnt = uni(s.incnt);
  s.bitbuf = (uint64_t)uni((uint32_t)s.bitbuf) | ((uint64_t)uni((uint32_t)(s.bitbuf >> 32)) << 32);
  s.bitcnt = (int)uni((uint32_t)s.bitcnt);
  s.err = (int)uni((uint32_t)s.err);
}

// the input block: lane l holds the dword at (aligned base) + 4 * (64 * blk + l); bytes outside the member's range are never loaded
struct InBlock { uint32_t word; uint32_t blk; uint32_t head; };   // head = (address of in[0]) & 3
__device__ inline void load_block(const State& s, InBlock& ib, uint32_t blk, int lane) {
  const int64_t q = (int64_t)(64ull * blk + (uint32_t)lane) * 4 - (int64_t)ib.head;   // offset of the dword's first byte from in[0]
  uint32_t w = 0;
  if (q >= 0 && q + 4 <= (int64_t)s.inlen) w = *(const uint32_t*)(s.in + q);
  else
    for (int j = 0; j < 4; j++)
      if (q + j >= 0 && q + j < (int64_t)s.inlen) w |= (uint32_t)s.in[q + j] << (8 * j);
  ib.word = w; ib.blk = blk;
}

// bitcnt > 32 behind it, unless the member's data ends first (the bits behind the end are zeros; every consumer checks bitcnt)
__device__ inline void refill(State& s, InBlock& ib, int lane) {
  while (s.bitcnt <= 32 && s.incnt < s.inlen) {
    const uint32_t v = s.incnt + ib.head, j = v >> 2;
    if ((j >> 6) != ib.blk) load_block(s, ib, j >> 6, lane);
    const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)ib.word, (int)uni(j & 63));
    if ((v & 3) == 0 && s.inlen - s.incnt >= 4) { s.bitbuf |= (uint64_t)w << s.bitcnt; s.bitcnt += 32; s.incnt += 4; }
    else { s.bitbuf |= (uint64_t)((w >> (8 * (v & 3))) & 0xffu) << s.bitcnt; s.bitcnt += 8; s.incnt += 1; }
  }
}

// `need` (<= 16) bits off a refilled buffer
__device__ inline uint32_t take(State& s, int need) {
  if (need > s.bitcnt) { s.err = LRA_BGZF_ERR_INPUT; return 0; }
  const uint32_t val = (uint32_t)s.bitbuf & ((1u << need) - 1u);
  s.bitbuf >>= need; s.bitcnt -= need;
  return val;
}

// the output of a member: ring position of member byte j is (j + shift) & RING_MASK, shift = (address of out[0]) & 3
struct Out {
  uint8_t* out; uint32_t outlen, outcnt, flushed, shift;
  uint8_t* ring;
};

// member bytes [o.flushed, upto) from the ring to `out`: whole aligned dwords, bytes at an unaligned end
__device__ inline void flush(Out& o, uint32_t upto, int lane) {
  const uint32_t va = o.flushed + o.shift, vb = upto + o.shift;          // in ring coordinates: out + (v - shift), out - shift is dword-aligned
  const uint32_t up = (va + 3) & ~3u, down = vb & ~3u;
  const uint32_t a = up < vb ? up : vb, b = down > a ? down : a;         // bytes [va, a), dwords [a, b), bytes [b, vb)
  uint8_t* base = o.out - o.shift;
  for (uint32_t v = va + lane; v < a; v += 64) base[v] = o.ring[v & RING_MASK];
  for (uint32_t v = a + 4 * lane; v < b; v += 256) *(uint32_t*)(base + v) = *(const uint32_t*)(o.ring + (v & RING_MASK));
  for (uint32_t v = b + lane; v < vb; v += 64) base[v] = o.ring[v & RING_MASK];
  o.flushed = upto;
}
__device__ inline void advance(Out& o, uint32_t n, int lane) {
  o.outcnt += n;
  if (o.outcnt - o.flushed >= PENDING) flush(o, ((o.outcnt + o.shift) & ~3u) - o.shift, lane);   // up to the last dword boundary of `out`
}

// a match of `len` bytes at `dist`: byte k is byte (k mod dist) of the source, which lies in front of the match
__device__ inline void copy_match(Out& o, uint32_t len, uint32_t dist, int lane) {
  const uint32_t v = o.outcnt + o.shift;
  if (dist + len <= RING) {                                               // the source is in the ring and the match does not overwrite it
    for (uint32_t k = lane; k < len; k += 64) {
      const uint32_t sk = dist >= len ? k : k % dist;
      o.ring[(v + k) & RING_MASK] = o.ring[(v - dist + sk) & RING_MASK];
    }
  } else {                                                                // dist > RING - 258 > len: written out by an earlier flush (at most PENDING + 258 bytes are pending)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");                // the other lanes' stores of that flush
    const uint8_t* src = o.out + o.outcnt - dist;
    for (uint32_t k = lane; k < len; k += 64) o.ring[(v + k) & RING_MASK] = src[k];
  }
}

__device__ inline void build_tables(WaveLds& L, int lane) {
  for (uint32_t e = lane; e < (1u << LIT_BITS); e += 64) {
    int len = 0;
    const int sym = walk_index(e, LIT_BITS, L.t.lencnt, L.t.lensym, &len);
    L.lit[e] = sym < 0 ? 0u : lit_entry(sym, len);
  }
  for (uint32_t e = lane; e < (1u << DIST_BITS); e += 64) {
    int len = 0;
    const int sym = walk_index(e, DIST_BITS, L.t.distcnt, L.t.distsym, &len);
    L.dist[e] = sym < 0 ? 0u : dist_entry(sym, len);
  }
}

// the symbols of one Huffman block (lra_infl_codes, with its order of checks)
__device__ inline int codes(State& s, InBlock& ib, Out& o, WaveLds& L, int lane) {
  for (;;) {
    refill(s, ib, lane);
    uint32_t e = uni(L.lit[(uint32_t)s.bitbuf & ((1u << LIT_BITS) - 1u)]);
    if ((e & 15u) == 0) {                                                 // a code of more than LIT_BITS bits, or none
      const int symbol = (int)uni((uint32_t)lra_infl_decode(s, L.t.lencnt, L.t.lensym));
      make_uniform(s);
      if (s.err) return s.err;
      e = lit_entry(symbol, 1);
    } else {
      take(s, (int)(e & 15u));
      if (s.err) return s.err;
    }
    const uint32_t kind = (e >> 8) & 3u;
    if (kind == K_LIT) {
      if (o.outcnt >= o.outlen) return LRA_BGZF_ERR_OUTPUT;
      if (lane == 0) o.ring[(o.outcnt + o.shift) & RING_MASK] = (uint8_t)(e >> 16);
      advance(o, 1, lane);
      continue;
    }
    if (kind == K_END) return LRA_BGZF_OK;
    if (kind == K_BAD) return LRA_BGZF_ERR_CODE;
    const uint32_t len = (e >> 16) + take(s, (int)((e >> 4) & 15u));
    if (s.err) return s.err;
    refill(s, ib, lane);
    uint32_t d = uni(L.dist[(uint32_t)s.bitbuf & ((1u << DIST_BITS) - 1u)]);
    if ((d & 15u) == 0) {
      const int ds = (int)uni((uint32_t)lra_infl_decode(s, L.t.distcnt, L.t.distsym));
      make_uniform(s);
      if (s.err) return s.err;
      d = dist_entry(ds, 1);
    } else {
      take(s, (int)(d & 15u));
      if (s.err) return s.err;
    }
    if ((d >> 8) & 3u) return LRA_BGZF_ERR_CODE;
    const uint32_t dist = (d >> 16) + take(s, (int)((d >> 4) & 15u));
    if (s.err) return s.err;
    if (dist > o.outcnt) return LRA_BGZF_ERR_DIST;
    if (len > o.outlen - o.outcnt) return LRA_BGZF_ERR_OUTPUT;
    copy_match(o, len, dist, lane);
    advance(o, len, lane);
  }
}

// a stored block (lra_infl_stored): the lanes copy its bytes into the ring
__device__ inline int stored(State& s, Out& o, int lane) {
  s.incnt -= (uint32_t)(s.bitcnt >> 3);
  s.bitbuf = 0; s.bitcnt = 0;
  if (s.inlen - s.incnt < 4) return LRA_BGZF_ERR_INPUT;
  const uint32_t len = uni(lra_le16(s.in + s.incnt)), nlen = uni(lra_le16(s.in + s.incnt + 2));
  s.incnt += 4;
  if (len != (~nlen & 0xffffu)) return LRA_BGZF_ERR_STORED;
  if (len > s.inlen - s.incnt) return LRA_BGZF_ERR_INPUT;
  if (len > o.outlen - o.outcnt) return LRA_BGZF_ERR_OUTPUT;
  for (uint32_t done = 0; done < len;) {
    const uint32_t n = len - done < 256 ? len - done : 256;
    const uint32_t v = o.outcnt + o.shift;
    for (uint32_t k = lane; k < n; k += 64) o.ring[(v + k) & RING_MASK] = s.in[s.incnt + k];
    s.incnt += n; done += n;
    advance(o, n, lane);
  }
  return LRA_BGZF_OK;
}

__global__ void __launch_bounds__(64 * WAVES) bgzf_inflate_lut(int n, const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                               const uint64_t* __restrict__ out_off, uint8_t* out, int32_t* __restrict__ status) {
  __shared__ WaveLds lds[WAVES];
  __shared__ uint32_t crc_tab[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) crc_tab[i] = lra_crc32_table_entry((uint32_t)i);
  __syncthreads();
  const int w = (int)uni(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const long b = (long)blockIdx.x * WAVES + w;
  if (b >= n) return;
  WaveLds& L = lds[w];
  const uint64_t i0 = in_off[b], o0 = out_off[b];
  const uint64_t ilen = in_off[b + 1] - i0, olen = out_off[b + 1] - o0;
  int rc = LRA_BGZF_OK;
  uint32_t expect = 0, total = 0, cdata = 0;
  if (lane == 0) {
    const uint8_t* src = in + i0;
    if (lra_bgzf_member(src, ilen, &total, &cdata) != 1 || total != ilen) rc = LRA_BGZF_ERR_HEADER;
    else if (lra_le32(src + total - 4) != olen || olen > 65536) rc = LRA_BGZF_ERR_ISIZE;
    else expect = lra_le32(src + total - 8);
  }
  rc = (int)uni((uint32_t)rc); expect = uni(expect); total = uni(total); cdata = uni(cdata);
  if (rc) { if (lane == 0) status[b] = rc; return; }

  State s;
  s.in = in + i0 + cdata; s.inlen = total - cdata - 8; s.incnt = 0; s.bitbuf = 0; s.bitcnt = 0; s.err = 0;
  InBlock ib;
  ib.head = (uint32_t)((uintptr_t)s.in & 3u); ib.blk = ~0u; ib.word = 0;
  Out o;
  o.out = out + o0; o.outlen = (uint32_t)olen; o.outcnt = 0; o.flushed = 0; o.shift = (uint32_t)((uintptr_t)o.out & 3u);
  o.ring = (uint8_t*)L.ring;
  int have = 0;                                                           // the codes in the lookup tables: 0 none, 1 fixed, 2 dynamic
  int last;
  do {
    refill(s, ib, lane);
    last = (int)take(s, 1);
    const int type = (int)take(s, 2);
    if (s.err) { rc = s.err; break; }
    if (type == 0) rc = stored(s, o, lane);
    else if (type == 1 || type == 2) {
      if (type == 2 || have != 1) {
        if (lane == 0) {
          if (type == 1) lra_infl_fixed_tables(L.t);
          else rc = lra_infl_dynamic_tables(s, L.t);
        }
        make_uniform(s);
        rc = (int)uni((uint32_t)rc);
        if (rc) break;
        build_tables(L, lane);
        have = type;
      }
      rc = codes(s, ib, o, L, lane);
    } else rc = LRA_BGZF_ERR_CODE;
  } while (rc == LRA_BGZF_OK && !last);
  if (!rc && o.outcnt != o.outlen) rc = LRA_BGZF_ERR_SIZE;
  flush(o, o.outcnt, lane);                                               // (a bad member's bytes so far, as bgzf_inflate leaves them: inside its range)
  if (rc) { if (lane == 0) status[b] = rc; return; }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");                  // the wave's output, read back across lanes
  const uint64_t slice = (olen + 63) / 64, lo = lane * slice < olen ? lane * slice : olen, hi = lo + slice < olen ? lo + slice : olen;
  uint32_t part = 0;
  if (hi > lo) part = lra_crc32_shift(lra_crc32_update(0, out + o0 + lo, hi - lo, crc_tab), olen - hi);
  for (int d = 32; d > 0; d >>= 1) part ^= (uint32_t)__shfl_xor((int)part, d);
  if (lane == 0) status[b] = part == expect ? LRA_BGZF_OK : LRA_BGZF_ERR_CRC;
}

}  // namespace

void lra_bgzf_launch_inflate_lut(hipStream_t st, int n, const uint8_t* in, const uint64_t* in_off, const uint64_t* out_off, uint8_t* out, int32_t* status) {
  if (n > 0) hipLaunchKernelGGL(bgzf_inflate_lut, dim3((unsigned)((n + WAVES - 1) / WAVES)), dim3(64 * WAVES), 0, st, n, in, in_off, out_off, out, status);
}

extern "C" int lra_bgzf_inflate_lut_batch(lra_ctx* ctx, int n_blocks, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_out_off, uint8_t* d_out,
                                          int32_t* d_status) {
  if (!ctx || n_blocks < 0 || (n_blocks && (!d_in || !d_in_off || !d_out_off || !d_out || !d_status))) return LRA_ERR_INVALID;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  lra_bgzf_launch_inflate_lut(ctx->stream, n_blocks, d_in, d_in_off, d_out_off, d_out, d_status);
  LRA_HIP_CHECK(ctx, hipGetLastError());
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return LRA_OK;
}

// lra_amd/csrc/md.hip -- the MD:Z value of a batch of alignments (lra --printMD; Alignment::PrintSAM :763-767) on the device (gfx950).
//
// The reference builds the alignment strings of the final blocks (CreateAlignmentStrings, Alignment.h:247-331) and re-parses them
// (AlignmentStringsToMD :204-245).  Both are restated here over the column stream the blocks define, without materialising it.  After
// toupper, every column (query char, text char; '-' on the gap side) is one of
//   M  text == query                         counted by the number in front of the next event
//   I  text == '-' != query                  consumed silently
//   X  text != query, neither is '-'         an event: <number><text char>
//   D  text != '-' == query                  a run of them is one event: <number>^<text chars>
// and the text is: for every event, the number of M columns since the previous X / D column, then the event; after the last column, the
// number once more if that column is M or I (the reference prints nothing behind a trailing mismatch or deletion).  The columns are
// compared as characters (a read's N against a reference A is a mismatch here, while the CIGAR's seqMap calls it a match).
//
// Shape: count, scan, emit.  An alignment is cut into SEGMENTS of MD_SEG_BLOCKS consecutive blocks (so a multi-Mb -CONTIG alignment of
// 10^5 blocks is hundreds of independent walks, not one); a GW-lane group walks a segment, GW columns per step, the column classes as
// ballot masks.  What crosses a segment boundary -- the M count in front of the first event, and whether a D at the segment's first
// column continues a run -- is resolved per alignment over its segments' summaries (md_resolve), the events' text lengths being known
// inside the segment.  Alignments whose blocks overlap (the walk's q / t leave the blocks' coordinates) are one segment each.
#include "common.h"
#include "scan.h"

namespace {

constexpr int MD_SEG_BLOCKS = 128;
constexpr int MD_GW = 16;                                    // lanes per segment walk (a noisy read's blocks are ~16 columns)
enum { CL_M = 0, CL_I = 1, CL_X = 2, CL_D = 3 };
enum { F_COLS = 1, F_XD = 2, F_FIRST_D = 4, F_FIRST_COL_D = 8 };

struct SegSum {                 // a segment walked with no carry (M count 0, no D before it)
  uint64_t bytes_rest;          // text of everything but the first event's number and its '^'
  uint32_t head_m, tail_m;      // M columns before the first X / D column (all of them when there is none); after the last one
  uint32_t flags, last_class;   // F_*; the class of the segment's last column
};
struct SegIn {                  // what md_resolve hands a segment for the emit walk
  uint64_t out;                 // byte offset of the segment's text inside its alignment's
  uint32_t carry_m, prev_d;     // M columns since the last X / D column in front of the segment; that column is a D directly before it
  uint32_t trailing, pad;       // the segment writes the alignment's trailing number
};

struct MdArgs {
  int n_aln;
  const int32_t* blocks; const uint64_t* block_off;
  const unsigned char* qseq; const uint64_t* q_off;
  const unsigned char* tseq; const uint64_t* t_off;
  uint32_t* n_seg; uint8_t* irregular;
  const uint64_t* seg_off; uint32_t* seg_aln; uint64_t n_segs;
  SegSum* sum; SegIn* in;
  uint64_t* len; const uint64_t* md_off; char* md;
};

__device__ __forceinline__ unsigned char up(unsigned char c) { return (c >= 'a' && c <= 'z') ? (unsigned char)(c - 32) : c; }
__device__ __forceinline__ int classify(unsigned char qc, unsigned char tc) {
  if (tc == qc) return CL_M;
  if (tc == '-') return CL_I;
  return qc == '-' ? CL_D : CL_X;
}
__device__ __forceinline__ int ndigits(uint32_t v) { int n = 1; while (v >= 10) { v /= 10; n++; } return n; }
__device__ __forceinline__ void put_num(char* p, uint32_t v, int n) { for (int k = n - 1; k >= 0; k--) { p[k] = (char)('0' + v % 10); v /= 10; } }

// segments per alignment (0 without blocks; 1 when its blocks overlap: the walk's q / t are then prefix sums from the first block on)
__global__ void __launch_bounds__(64) md_segments(MdArgs A) {
  const int lane = threadIdx.x;
  for (int a = blockIdx.x; a < A.n_aln; a += gridDim.x) {
    const long nb = (long)(A.block_off[a + 1] - A.block_off[a]);
    const int32_t* B = A.blocks + 3 * A.block_off[a];
    bool irr = false;
    for (long base = 0; base < nb - 1 && !irr; base += 64) {
      const long i = base + lane;
      bool x = false;
      if (i < nb - 1) {
        const long bl = B[3 * i + 2];
        const long qg = (long)B[3 * i + 3] - B[3 * i] - bl, tg = (long)B[3 * i + 4] - B[3 * i + 1] - bl;
        x = bl < 0 || qg < 0 || tg < 0;
      }
      irr = __ballot(x) != 0ULL;
    }
    if (lane == 0) {
      A.irregular[a] = irr ? 1 : 0;
      A.n_seg[a] = nb == 0 ? 0u : irr ? 1u : (uint32_t)((nb + MD_SEG_BLOCKS - 1) / MD_SEG_BLOCKS);
    }
  }
}

__global__ void md_seg_fill(MdArgs A) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= A.n_aln) return;
  for (uint64_t s = A.seg_off[a]; s < A.seg_off[a + 1]; s++) A.seg_aln[s] = (uint32_t)a;
}

// One segment's walk.  EMIT = false: its summary with no carry; EMIT = true: its text at `out` from the carry md_resolve found.
template <bool EMIT>
__global__ void __launch_bounds__(64) md_walk(MdArgs A) {
  constexpr int GW = MD_GW, GPW = 64 / GW;
  const int lane = threadIdx.x & (GW - 1), gbase = threadIdx.x - lane;
  const unsigned long long gmask = ~0ULL >> (64 - GW);
  const unsigned long long below = (1ULL << lane) - 1;
  auto BAL = [&](bool x) -> unsigned long long { return (__ballot(x) >> gbase) & gmask; };
  for (uint64_t s = (uint64_t)blockIdx.x * GPW + (uint64_t)threadIdx.x / GW; s < A.n_segs; s += (uint64_t)gridDim.x * GPW) {
    const int a = (int)A.seg_aln[s];
    const uint64_t k = s - A.seg_off[a];
    const long nb = (long)(A.block_off[a + 1] - A.block_off[a]);
    const int32_t* B = A.blocks + 3 * A.block_off[a];
    const unsigned char* R = A.qseq + A.q_off[a];
    const unsigned char* G = A.tseq + A.t_off[a];
    const long b0 = A.irregular[a] ? 0 : (long)k * MD_SEG_BLOCKS;
    const long b1 = A.irregular[a] ? nb : min(nb, b0 + MD_SEG_BLOCKS);
    uint32_t m = 0; bool prevD = false;
    char* out = nullptr; const char* lim = nullptr;                  // (lim: the alignment's end -- nothing is written past it, whatever the counts say)
    if (EMIT) { const SegIn in = A.in[s]; m = in.carry_m; prevD = in.prev_d != 0; out = A.md + A.md_off[a] + in.out; lim = A.md + A.md_off[a + 1]; }
    uint64_t bytes = 0;
    uint32_t head_m = 0, flags = 0, firstTok = 0; int lastClass = CL_M;
    // GW columns of one piece: pairs (both sides read), insertions (text '-'), deletions (query '-')
    auto chunk = [&](int kind, long q, long t, int cnt) {
      int cls = CL_M; unsigned char tc = 0;
      if (lane < cnt) {
        const unsigned char qc = kind == CL_D ? (unsigned char)'-' : up(R[q + lane]);
        tc = kind == CL_I ? (unsigned char)'-' : up(G[t + lane]);
        cls = classify(qc, tc);
      }
      const unsigned long long valid = (cnt >= 64) ? ~0ULL : ((1ULL << cnt) - 1);
      const unsigned long long Mm = BAL(lane < cnt && cls == CL_M), Xm = BAL(lane < cnt && cls == CL_X), Dm = BAL(lane < cnt && cls == CL_D);
      const unsigned long long xd = Xm | Dm;
      const unsigned long long dstart = Dm & ~((Dm << 1) | (prevD ? 1ULL : 0ULL));
      const unsigned long long ev = (Xm | dstart) & valid, dcont = Dm & ~dstart;
      uint32_t tok = 0, num = 0; int nd = 0;
      if ((ev >> lane) & 1ULL) {
        const unsigned long long p = xd & below;                          // X / D columns in front of this one, inside the chunk
        const unsigned long long from = p ? ~((2ULL << (63 - __clzll((long long)p))) - 1) : ~0ULL;
        num = (p ? 0u : m) + (uint32_t)__popcll(Mm & below & from);
        nd = ndigits(num);
        tok = (uint32_t)nd + (cls == CL_X ? 1u : 2u);
      } else if ((dcont >> lane) & 1ULL) tok = 1;
      if (!EMIT && !(flags & F_XD) && xd) {                               // the segment's first X / D column: its number and '^' are md_resolve's
        const int f = __ffsll((long long)xd) - 1;
        const uint32_t hm = m + (uint32_t)__popcll(Mm & ((1ULL << f) - 1));
        const bool isD = (Dm >> f) & 1ULL;
        head_m = hm;
        flags |= F_XD | (isD ? F_FIRST_D : 0) | ((isD && f == 0 && !(flags & F_COLS)) ? F_FIRST_COL_D : 0);
        firstTok = (uint32_t)ndigits(hm) + (isD ? 2u : 1u);
      }
      // exclusive prefix of the tokens' lengths inside the group
      uint32_t inc = tok;
      for (int d = 1; d < GW; d <<= 1) { const uint32_t y = __shfl_up(inc, d, GW); if (lane >= d) inc += y; }
      const uint32_t total = __shfl(inc, GW - 1, GW);
      if (EMIT && tok && out + bytes + inc <= lim) {
        char* w = out + bytes + (inc - tok);
        if ((ev >> lane) & 1ULL) { put_num(w, num, nd); w += nd; if (cls == CL_D) *w++ = '^'; }
        *w = (char)tc;
      }
      bytes += total;
      if (xd) m = (uint32_t)__popcll(Mm & ~((2ULL << (63 - __clzll((long long)xd))) - 1));
      else m += (uint32_t)__popcll(Mm);
      if (!EMIT && !(flags & F_XD)) head_m = m;
      lastClass = __shfl(cls, cnt - 1, GW);
      prevD = lastClass == CL_D;
      flags |= F_COLS;
    };
    auto piece = [&](int kind, long q, long t, long len) { for (long o = 0; o < len; o += GW) chunk(kind, q + o, t + o, (int)min((long)GW, len - o)); };
    if (b0 < b1) {
      long q = B[3 * b0], t = B[3 * b0 + 1];
      for (long i = b0; i < b1; i++) {
        const long bl = B[3 * i + 2];
        const long L = bl > 0 ? bl : 0;
        piece(CL_M, q, t, L); q += L; t += L;
        if (i + 1 >= nb) continue;
        long qg = (long)B[3 * i + 3] - B[3 * i] - bl, tg = (long)B[3 * i + 4] - B[3 * i + 1] - bl;
        if (qg > 0 || tg > 0) {
          const long c = qg < tg ? qg : tg;
          qg -= c; tg -= c;
          piece(CL_I, q, t, qg); q += qg;
          piece(CL_D, q, t, tg); t += tg;
          if (c > 0) { piece(CL_M, q, t, c); q += c; t += c; }
        }
      }
    }
    if (EMIT) {
      if (A.in[s].trailing && lane == 0 && out + bytes + ndigits(m) <= lim) put_num(out + bytes, m, ndigits(m));
    } else if (lane == 0) {
      SegSum r;
      r.bytes_rest = bytes - ((flags & F_XD) ? firstTok : 0u); r.head_m = head_m; r.tail_m = m; r.flags = flags; r.last_class = (uint32_t)lastClass;
      A.sum[s] = r;
    }
  }
}

// Per alignment, its segments in order: the carry into each, the offset of its text, the alignment's length.
__global__ void md_resolve(MdArgs A) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= A.n_aln) return;
  uint64_t at = 0; uint32_t m = 0; int last = -1; long lastSeg = -1;
  for (uint64_t s = A.seg_off[a]; s < A.seg_off[a + 1]; s++) {
    const SegSum r = A.sum[s];
    SegIn in; in.out = at; in.carry_m = m; in.prev_d = last == CL_D ? 1u : 0u; in.trailing = 0; in.pad = 0;
    A.in[s] = in;
    if (!(r.flags & F_COLS)) continue;
    if (r.flags & F_XD) {
      const bool cont = (r.flags & F_FIRST_COL_D) && last == CL_D;
      if (cont) at += 1;
      else { uint32_t v = m + r.head_m, n = 1; while (v >= 10) { v /= 10; n++; } at += n + ((r.flags & F_FIRST_D) ? 2u : 1u); }
      at += r.bytes_rest;
      m = r.tail_m;
    } else m += r.head_m;
    last = (int)r.last_class; lastSeg = (long)s;
  }
  if (lastSeg >= 0 && (last == CL_M || last == CL_I)) {
    A.in[lastSeg].trailing = 1;
    uint32_t v = m, n = 1; while (v >= 10) { v /= 10; n++; }
    at += n;
  }
  A.len[a] = at;
}

}  // namespace

extern "C" int lra_md_strings_batch(lra_ctx* ctx, int n_aln, const int32_t* d_blocks, const uint64_t* d_block_off, const char* d_qseq, const uint64_t* d_q_off,
                                    const int32_t* d_q_len, const char* d_tseq, const uint64_t* d_t_off, lra_md_result* out) {
  (void)d_q_len;
  if (!ctx || !out || n_aln < 0 || (n_aln > 0 && (!d_blocks || !d_block_off || !d_qseq || !d_q_off || !d_tseq || !d_t_off))) return LRA_ERR_INVALID;
  memset(out, 0, sizeof(*out));
  out->n_aln = n_aln;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t nA = (size_t)n_aln;
  auto sz = [](size_t n, size_t e) { return (n * e + 255) & ~(size_t)255; };
  // 184: per alignment (segment counts, the irregular flags, segment offsets, lengths, MD offsets -- the offsets are the result's); 185: per segment; 186: the text
  char* w = (char*)lra_ensure(ctx, 184, sz(nA, 4) + sz(nA, 1) + sz(nA + 1, 8) * 3 + sz(nA, 8) + 4096);
  if (!w) return LRA_ERR_NOMEM;
  MdArgs A; memset(&A, 0, sizeof A);
  A.n_aln = n_aln; A.blocks = d_blocks; A.block_off = d_block_off;
  A.qseq = (const unsigned char*)d_qseq; A.q_off = d_q_off; A.tseq = (const unsigned char*)d_tseq; A.t_off = d_t_off;
  A.n_seg = (uint32_t*)w; w += sz(nA, 4);
  A.irregular = (uint8_t*)w; w += sz(nA, 1);
  uint64_t* seg_off = (uint64_t*)w; w += sz(nA + 1, 8);
  A.len = (uint64_t*)w; w += sz(nA, 8);
  uint64_t* md_off = (uint64_t*)w; w += sz(nA + 1, 8);
  A.seg_off = seg_off; A.md_off = md_off;
  if (n_aln == 0) {
    LRA_HIP_CHECK(ctx, hipMemsetAsync(md_off, 0, 8, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    out->d_md_off = md_off;
    return LRA_OK;
  }
  lra_time_begin(ctx, "md");
  hipLaunchKernelGGL(md_segments, dim3((unsigned)std::min<size_t>(nA, (size_t)ctx->num_cu * 32)), dim3(64), 0, st, A);
  if (lra_exclusive_scan<uint32_t>(ctx, (long)n_aln, A.n_seg, seg_off)) return LRA_ERR_HIP;
  uint64_t nS = 0;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&nS, seg_off + n_aln, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  A.n_segs = nS;
  char* ws = (char*)lra_ensure(ctx, 185, sz(nS + 1, 4) + sz(nS + 1, sizeof(SegSum)) + sz(nS + 1, sizeof(SegIn)) + 4096);
  if (!ws) return LRA_ERR_NOMEM;
  A.seg_aln = (uint32_t*)ws; ws += sz(nS + 1, 4);
  A.sum = (SegSum*)ws; ws += sz(nS + 1, sizeof(SegSum));
  A.in = (SegIn*)ws;
  const unsigned walkGrid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((nS + 3) / 4, (uint64_t)ctx->num_cu * 64));
  hipLaunchKernelGGL(md_seg_fill, dim3((n_aln + 255) / 256), dim3(256), 0, st, A);
  if (nS) hipLaunchKernelGGL(md_walk<false>, dim3(walkGrid), dim3(64), 0, st, A);
  hipLaunchKernelGGL(md_resolve, dim3((n_aln + 255) / 256), dim3(256), 0, st, A);
  if (lra_exclusive_scan<uint64_t>(ctx, (long)n_aln, A.len, md_off)) return LRA_ERR_HIP;
  uint64_t total = 0;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&total, md_off + n_aln, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  char* md = (char*)lra_ensure(ctx, 186, total + 64);
  if (!md) return LRA_ERR_NOMEM;
  A.md = md;
  if (nS) hipLaunchKernelGGL(md_walk<true>, dim3(walkGrid), dim3(64), 0, st, A);
  lra_time_end(ctx);
  LRA_HIP_CHECK(ctx, hipGetLastError());
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  out->n_bytes = total; out->d_md_off = md_off; out->d_md = md;
  return LRA_OK;
}

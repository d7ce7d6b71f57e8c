// lra_amd/csrc/bam_depth.hip -- lra_bam_depth: the coverage of a coordinate-sorted BAM file, per base or per bin, whole or for a region (gfx950).
// include/lra_hip.h has the interface and the rules; bam_pass.h is the pass it shares with lra_bam_view (the windows, a region's plan, the refusals) and
// the record front in front of dp_select (Front, rec_check, rec_in_region, rec_cut) with the handle shell.
//
// records.  The pass's front: rec_check, a lane per framed record: the record's arithmetic; bs_span gives a region pass every record's span for the overlap
// test.  dp_select, a lane per record: the order against the record in front (the carried key for the first), the filter (refID, flag, mapq, and
// rec_in_region's overlap and first record at or behind the region's end; rec_cut behind it), and where the ops are: the core CIGAR, or the CG:B:I tag
// found by the aux walk when the core CIGAR is <l_seq>S<n>N.  One scan of the op counts.
// ops.  dp_oplen, a lane per op: its reference length (M D N = X), the op code against 8.  One scan over the ops; less its value at the record's first
// op it is the op's offset from the record's pos.  dp_ends, a lane per record: pos + the reference length of its ops.
// accumulate.  dp_accum, a lane per op, adds to the difference array diff[] of the position window [dbase, dbase + span): + 1 where a maximal run of
// covered ops begins, - 1 behind its last base -- a covered op whose reference-consuming neighbour in the record is covered too adds nothing, so = X =
// runs cost one pair of integer atomics per gap, not per op.  Integer adds commute: the array is the same whatever order the lanes run in.
// the window of positions.  The host plans a window's records (their ref, clamped start and end come back in one copy) into tasks: finish the
// positions below the next record's start, slide the array when a record reaches beyond it (or double it when one record is longer), accumulate a
// position-ordered prefix of the records, and so on.  The tasks run lazily, one delivered piece per call.
// finish.  One scan of diff over the piece, dp_depth adds the carried running depth, clears the cells and reduces the stats; bins: a second scan of
// the depths, dp_bins takes each bin's sum as a difference of two prefix sums (the bin a piece cuts carries its partial sum to the next piece).
// text.  dp_linelen / dp_binlen, a lane per position / bin: the line's length from the name's length and the digits; one scan places the lines;
// dp_lines / dp_binlines write them.  Stretches no record reaches cost nothing in the default mode (the base jumps) and no diff traffic in the others.
#include "common.h"
#include "scan.h"
#include "bam_pass.h"
#include "bam_keys.h"
#include <algorithm>
#include <deque>
#include <vector>

namespace {

constexpr uint64_t MIN_SPAN = 65536, DEFAULT_SPAN = 4ull << 20;
constexpr uint64_t PIECE_POS = 4ull << 20;                    // positions (or bins) of one piece at most: 16 MiB of values
constexpr uint64_t PIECE_TEXT = 64ull << 20;                  // and the bytes of its text
constexpr uint32_t DEFAULT_EXCLUDE = 0x704;

enum { B_ORDER = B_OWN, B_AUX, B_OP };                         // bad[] behind the pass's words: the lowest record out of order, with a bad aux block, with a bad op code

struct Dp {                                                   // what the kernels of a window see
  Front F;                                                    // (bam_pass.h) record i is F.data[F.pos[i], F.pos[i + 1])
  uint32_t req, excl, min_mapq, count_del;
  uint32_t last_ref; int32_t last_pos; int has_last;          // the key of the record in front of the window's first
  uint32_t* keep;
  int32_t* r_ref; int32_t* r_pos; int64_t* r_end;
  uint32_t* c_op; uint64_t* op_off; uint64_t* ops_src;
  uint32_t* oplen; uint64_t* ostart; uint64_t n_op;
};

__device__ __forceinline__ bool consumes_ref(uint32_t code) { return (0x18du >> code) & 1u; }            // M D N = X
__device__ __forceinline__ bool covers(uint32_t code, uint32_t count_del) { return code == 0 || code == 7 || code == 8 || (code == 2 && count_del); }

__global__ void __launch_bounds__(256) dp_select(Dp V) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V.F.n) return;
  const uint64_t at0 = V.F.pos[i];
  const uint8_t* p = V.F.data + at0;
  const Core c = core_of(p);
  // the order: (refID, pos) with refID -1 last
  uint32_t pr = 0; int32_t pp = 0; bool has = false;
  if (i) { const uint8_t* q = V.F.data + V.F.pos[i - 1]; pr = le32(q + 4); pp = (int32_t)le32(q + 8); has = true; }
  else if (V.has_last) { pr = V.last_ref; pp = V.last_pos; has = true; }
  if (has && ((uint32_t)c.ref < pr || ((uint32_t)c.ref == pr && c.pos < pp))) atomicMin(&V.F.bad[B_ORDER], (unsigned long long)i);
  bool keep = c.ref >= 0 && (c.flag & V.req) == V.req && (c.flag & V.excl) == 0 && c.mapq >= V.min_mapq;
  if (V.F.region) keep = rec_in_region(V.F, i, c.ref, c.pos) && keep;
  uint64_t ops = at0 + 36 + c.l_name; uint32_t n_op = c.n_cig;
  if (keep && !ops_of(V.F.data, at0, V.F.pos[i + 1], c, &ops, &n_op)) { atomicMin(&V.F.bad[B_AUX], (unsigned long long)i); keep = false; }   // (the CG:B:I tag's, if the record has one)
  V.keep[i] = keep ? 1u : 0u; V.c_op[i] = keep ? n_op : 0u; V.ops_src[i] = ops;
  V.r_ref[i] = c.ref; V.r_pos[i] = c.pos;
}

__global__ void __launch_bounds__(256) dp_oplen(Dp V) {
  const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= V.n_op) return;
  const uint64_t r = last_le(V.op_off, V.F.n, o);
  const uint32_t op = le32(V.F.data + V.ops_src[r] + 4 * (o - V.op_off[r]));
  const uint32_t code = op & 15u;
  if (code > 8u) atomicMin(&V.F.bad[B_OP], (unsigned long long)r);
  V.oplen[o] = code <= 8u && consumes_ref(code) ? op >> 4 : 0u;
}

// a lane per record: the end of its ops on the reference
__global__ void __launch_bounds__(256) dp_ends(Dp V) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V.F.n) return;
  int64_t e = (int64_t)V.r_pos[i];
  if (V.keep[i]) e += (int64_t)(V.ostart[V.op_off[i + 1]] - V.ostart[V.op_off[i]]);
  V.r_end[i] = e;
}

struct Acc {
  int32_t* diff; int64_t dbase; uint64_t cells;               // diff[k] is position dbase + k; `cells` of them may be written
  int64_t lo_c, hi_c;
  uint64_t o_lo, o_hi;
  unsigned int* outside;                                      // adds that fell outside the array (none, by the plan)
};

__global__ void __launch_bounds__(256) dp_accum(Dp V, Acc A) {
  const uint64_t o = A.o_lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= A.o_hi) return;
  const uint32_t len = V.oplen[o];
  if (!len) return;                                            // (consumes no reference base)
  const uint64_t r = last_le(V.op_off, V.F.n, o), o0 = V.op_off[r], o1 = V.op_off[r + 1];
  const uint8_t* src = V.F.data + V.ops_src[r];
  if (!covers(le32(src + 4 * (o - o0)) & 15u, V.count_del)) return;
  // the reference-consuming neighbours: the ops of no reference length in between are the short look
  bool left = false, right = false;
  for (uint64_t k = o; k > o0; k--) if (V.oplen[k - 1]) { left = covers(le32(src + 4 * (k - 1 - o0)) & 15u, V.count_del); break; }
  for (uint64_t k = o + 1; k < o1; k++) if (V.oplen[k]) { right = covers(le32(src + 4 * (k - o0)) & 15u, V.count_del); break; }
  const int64_t s = (int64_t)V.r_pos[r] + (int64_t)(V.ostart[o] - V.ostart[o0]), e = s + (int64_t)len;
  if (!left) {
    const int64_t p = max(s, A.lo_c);
    if (p < A.hi_c) {
      const int64_t k = p - A.dbase;
      if (k >= 0 && (uint64_t)k < A.cells) atomicAdd(&A.diff[k], 1); else if (k >= 0) atomicAdd(A.outside, 1u);
    }
  }
  if (!right) {
    const int64_t p = max(e, A.lo_c);
    if (p < A.hi_c) {
      const int64_t k = p - A.dbase;
      if (k >= 0 && (uint64_t)k < A.cells) atomicAdd(&A.diff[k], -1); else if (k >= 0) atomicAdd(A.outside, 1u);
    }
  }
}

// the live cells [from, from + n) of src move to dst[0, n); src is left clear
__global__ void __launch_bounds__(256) dp_slide(int32_t* __restrict__ dst, int32_t* __restrict__ src, uint64_t from, uint64_t n) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  dst[k] = src[from + k]; src[from + k] = 0;
}

struct Fin {
  int32_t* diff; const uint64_t* off; uint64_t m;             // the piece's cells diff[0, m) and their exclusive scan; diff null: a stretch of zeros
  uint32_t carry;                                             // the running depth in front of the piece
  uint32_t* depth;                                            // [m]
  unsigned long long* red;                                    // [0] positions with depth > 0, [1] the sum of depth, [2] its maximum
  int64_t first; int32_t ref; int all;
  const char* rname; const uint64_t* rname_off;
  uint32_t* llen; const uint64_t* loff; unsigned char* text;
  // bins
  const uint64_t* psum;                                       // the exclusive scan of depth[0, m) (null: zeros)
  int64_t b0, range_end; uint64_t bin, k0, nb; unsigned long long part;
  unsigned long long* sum;                                    // [nb]
};

// a grid-stride lane per position; the stats leave a block as one set of atomics (a set per wave was most of the kernel: three addresses, 16 K waves)
__global__ void __launch_bounds__(256) dp_depth(Fin F) {
  __shared__ unsigned long long sh_cov[4], sh_sum[4]; __shared__ uint32_t sh_max[4];
  unsigned long long cov = 0, s = 0; uint32_t mx = 0;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < F.m; k += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t d = F.carry + (uint32_t)F.off[k] + (uint32_t)F.diff[k];
    F.depth[k] = d; F.diff[k] = 0;
    cov += d ? 1 : 0; s += d; mx = max(mx, d);
  }
  for (int o = 32; o > 0; o >>= 1) { cov += __shfl_xor(cov, o); s += __shfl_xor(s, o); mx = max(mx, (uint32_t)__shfl_xor((int)mx, o)); }
  if ((threadIdx.x & 63) == 0) { sh_cov[threadIdx.x >> 6] = cov; sh_sum[threadIdx.x >> 6] = s; sh_max[threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) { cov += sh_cov[w]; s += sh_sum[w]; mx = max(mx, sh_max[w]); }
    if (cov) { atomicAdd(&F.red[0], cov); atomicAdd(&F.red[1], s); atomicMax(&F.red[2], (unsigned long long)mx); }
  }
}

__device__ __forceinline__ uint32_t ref_name_len(const Fin& F) { return (uint32_t)(F.rname_off[F.ref + 1] - F.rname_off[F.ref]); }
__device__ __forceinline__ unsigned char* put_ref_name(const Fin& F, unsigned char* d) {
  const uint64_t a = F.rname_off[F.ref], b = F.rname_off[F.ref + 1];
  for (uint64_t k = a; k < b; k++) *d++ = (unsigned char)F.rname[k];
  return d;
}

__global__ void __launch_bounds__(256) dp_linelen(Fin F) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= F.m) return;
  const uint32_t d = F.diff ? F.depth[k] : 0u;
  F.llen[k] = d || F.all ? ref_name_len(F) + 3u + (uint32_t)ndig((uint64_t)(F.first + (int64_t)k + 1)) + (uint32_t)ndig(d) : 0u;
}

__global__ void __launch_bounds__(256) dp_lines(Fin F) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= F.m || F.loff[k + 1] == F.loff[k]) return;
  unsigned char* d = put_ref_name(F, F.text + F.loff[k]);
  *d++ = '\t'; d = put_u(d, (uint64_t)(F.first + (int64_t)k + 1));
  *d++ = '\t'; d = put_u(d, F.diff ? F.depth[k] : 0u);
  *d = '\n';
}

// a lane per bin the piece touches: the sum of its positions inside the piece, the first bin's with the part the piece in front left
__global__ void __launch_bounds__(256) dp_bins(Fin F) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= F.nb) return;
  const int64_t bs = F.b0 + (int64_t)((F.k0 + j) * F.bin), be = min(bs + (int64_t)F.bin, F.range_end);
  const int64_t s = max(bs, F.first), e = min(be, F.first + (int64_t)F.m);
  unsigned long long v = j == 0 ? F.part : 0ull;
  if (F.psum && e > s) v += F.psum[e - F.first] - F.psum[s - F.first];
  F.sum[j] = v;
}

__device__ __forceinline__ unsigned long long mean_hundredths(unsigned long long sum, unsigned long long len) { return (100ull * sum + len / 2) / len; }

__global__ void __launch_bounds__(256) dp_binlen(Fin F) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= F.nb) return;
  const int64_t bs = F.b0 + (int64_t)((F.k0 + j) * F.bin), be = min(bs + (int64_t)F.bin, F.range_end);
  const unsigned long long h = mean_hundredths(F.sum[j], (unsigned long long)(be - bs));
  F.llen[j] = ref_name_len(F) + 4u + (uint32_t)ndig((uint64_t)bs) + (uint32_t)ndig((uint64_t)be) + (uint32_t)ndig(h / 100) + 3u;
}

__global__ void __launch_bounds__(256) dp_binlines(Fin F) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= F.nb) return;
  const int64_t bs = F.b0 + (int64_t)((F.k0 + j) * F.bin), be = min(bs + (int64_t)F.bin, F.range_end);
  const unsigned long long h = mean_hundredths(F.sum[j], (unsigned long long)(be - bs));
  unsigned char* d = put_ref_name(F, F.text + F.loff[j]);
  *d++ = '\t'; d = put_u(d, (uint64_t)bs);
  *d++ = '\t'; d = put_u(d, (uint64_t)be);
  *d++ = '\t'; d = put_u(d, h / 100);
  *d++ = '.'; *d++ = (unsigned char)('0' + (h % 100) / 10); *d++ = (unsigned char)('0' + h % 10);
  *d = '\n';
}

enum { T_FINISH, T_NEWREF, T_SLIDE, T_ACCUM };
struct Task { int kind; int64_t a, b, c; };                   // FINISH: a = to; NEWREF: a = ref; SLIDE: a = the span behind it; ACCUM: ops [a, b), c = the live end behind it

}  // namespace

struct lra_bam_depth : lra_bam_pass {
  lra_bam_depth_opts O{};
  uint64_t span = 0, max_line = 0;
  // the pass: the state the queued tasks have reached, and (pl_) the state they will have reached when all have run
  int32_t cur_ref = -1; int64_t base = 0, dbase = 0, live = 0; uint32_t carry = 0; uint64_t bin_part = 0;
  int32_t pl_ref = -1; int64_t pl_base = 0, pl_dbase = 0, pl_live = 0, pl_last = 0; uint64_t pl_span = 0;   // pl_last: the last counted record's start
  bool have_last = false; uint32_t last_ref = 0; int32_t last_pos = 0;
  bool w_have = false; uint32_t w_ref = 0; int32_t w_pos = 0; uint64_t w_n = 0, w_kept = 0;   // the window in hand
  std::deque<Task> tasks; std::vector<Task> w_tasks;
  bool dirty = false, flushed = false, done = true;           // diff holds adds; the last tasks are queued; the pass delivers nothing more
  Dp V{};
  // the window's arrays, the position window, the piece
  Buf<uint32_t> keep, c_op, oplen, depth, llen; Buf<int32_t> r_ref, r_pos, dbuf[2]; Buf<int64_t> r_end;
  Buf<uint64_t> op_off, ops_src, ostart, doff, psum, loff; Buf<unsigned long long> sum; Buf<uint8_t> text;
  int dcur = 0;
  PinBuf<char> h_meta, h_text; PinBuf<uint32_t> h_depth; PinBuf<uint64_t> h_sum;
  struct lra_bam_depth_stats S{};

  void release_all() {
    release_pass();
    keep.release(); c_op.release(); oplen.release(); depth.release(); llen.release();
    r_ref.release(); r_pos.release(); dbuf[0].release(); dbuf[1].release(); r_end.release(); op_off.release(); ops_src.release(); ostart.release();
    doff.release(); psum.release(); loff.release(); sum.release(); text.release();
    h_meta.release(); h_text.release(); h_depth.release(); h_sum.release();
  }
  int64_t range_lo(int32_t ref) const { return mode == 2 && ref == ref_id ? beg : 0; }
  int64_t range_hi(int32_t ref) const { return mode == 2 ? (ref == ref_id ? end : 0) : (int64_t)refs.len[(size_t)ref]; }
  bool prints_zeros() const { return O.bin || O.all_positions; }
  bool clear_diff(Buf<int32_t>& b, uint64_t cells) {           // a zeroed array of at least `cells`
    if (b.n >= cells && !dirty) return true;
    if (!grab(b, cells)) return false;
    return hipMemsetAsync(b.p, 0, b.n * sizeof(int32_t), ctx->stream) == hipSuccess;
  }
  int begin_pass();
  // the pass's consumer
  int window(uint64_t n, uint64_t limit, uint64_t* bad_idx, uint64_t* bad_pos, std::string* bad_why, uint64_t* stop_idx);
  void forget() { w_tasks.clear(); w_have = false; w_n = w_kept = 0; }
  bool deliver() {
    for (const Task& t : w_tasks) tasks.push_back(t);
    w_tasks.clear();
    // a fault ends the pass behind this window: what lies below the last counted record's start is final and goes first
    if (!pend_err.empty() && pl_ref >= 0 && pl_last > pl_base) { tasks.push_back(Task{T_FINISH, pl_last, 0, 0}); pl_base = pl_last; }
    if (w_have) { have_last = true; last_ref = w_ref; last_pos = w_pos; }
    if (!chunk_open) have_last = false;                        // (a region's next chunk may start in front of what this window read behind its limit)
    S.records_read += w_n; S.records_counted += w_kept; S.records_filtered += w_n - w_kept;
    return !tasks.empty();
  }
  void plan_newref(std::vector<Task>& out, int32_t ref);
  void plan_until_ref(std::vector<Task>& out, int32_t ref);
  int run_task(struct lra_bam_depth_piece* piece, bool* made);
  int finish_piece(int64_t to, struct lra_bam_depth_piece* piece, bool* made);
  int next(struct lra_bam_depth_piece* piece);
};

int lra_bam_depth::begin_pass() {
  hipStream_t st = ctx->stream;
  tasks.clear(); w_tasks.clear(); have_last = false; w_have = false; flushed = false; done = false;
  cur_ref = pl_ref = -1; base = dbase = live = pl_base = pl_dbase = pl_live = 0; carry = 0; bin_part = 0; pl_span = span;
  LRA_HIP_CHECK(ctx, hipMemsetAsync(misc.p + MISC_CNT, 0, 32, st));
  if (dirty || dbuf[0].n < span + 2 || dbuf[1].n < span + 2) {   // a pass that was left, or the first one: both arrays are cleared
    dirty = true;
    if (!clear_diff(dbuf[0], span + 2) || !clear_diff(dbuf[1], span + 2)) return fail(LRA_ERR_NOMEM, "lra_bam_depth: hipMalloc failed for a position window of %llu bases", (unsigned long long)span);
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    dirty = false;
  }
  if (mode == 2) { std::vector<Task> t; plan_newref(t, ref_id); for (const Task& x : t) tasks.push_back(x); }
  return LRA_OK;
}

void lra_bam_depth::plan_newref(std::vector<Task>& out, int32_t ref) {
  out.push_back(Task{T_NEWREF, ref, 0, 0});
  pl_ref = ref; pl_base = pl_dbase = pl_live = pl_last = range_lo(ref);
}

// the references in front of `ref` (n_ref: all that remain) are finished: the one in hand to its end, the ones without records as zeros where they print
void lra_bam_depth::plan_until_ref(std::vector<Task>& out, int32_t ref) {
  if (pl_ref >= 0) { out.push_back(Task{T_FINISH, range_hi(pl_ref), 0, 0}); pl_base = range_hi(pl_ref); }
  if (mode == 2) return;
  for (int32_t r = pl_ref + 1; r < ref; r++) {
    if (!prints_zeros()) continue;
    plan_newref(out, r);
    out.push_back(Task{T_FINISH, range_hi(r), 0, 0}); pl_base = range_hi(r);
  }
  if (ref >= refs.n_ref) pl_ref = refs.n_ref - 1;
}

int lra_bam_depth::window(uint64_t n, uint64_t limit, uint64_t* bad_idx, uint64_t* bad_pos, std::string* bad_why, uint64_t* stop_idx) {
  hipStream_t st = ctx->stream;
  *bad_idx = NONE; *stop_idx = NONE;
  forget();
  memset(&V, 0, sizeof V);
  V.req = O.require; V.excl = O.exclude; V.min_mapq = O.min_mapq; V.count_del = O.count_deletions;
  V.last_ref = last_ref; V.last_pos = last_pos; V.has_last = have_last;
  if (!(grab(keep, n) && grab(c_op, n) && grab(op_off, n + 1) && grab(ops_src, n) && grab(r_ref, n) && grab(r_pos, n) && grab(r_end, n)))
    return fail(LRA_ERR_NOMEM, "lra_bam_depth: hipMalloc failed for the arrays of %llu records", (unsigned long long)n);
  V.keep = keep.p; V.r_ref = r_ref.p; V.r_pos = r_pos.p; V.r_end = r_end.p;
  V.c_op = c_op.p; V.op_off = op_off.p; V.ops_src = ops_src.p;
  unsigned long long res[B_WORDS];
  uint64_t n_op = 0;
  {
    Timer T(st);
    const int rc = front_check(V.F, n, limit, bad_idx, bad_pos, bad_why);
    if (rc || *bad_idx != NONE) { S.ms_frame_select += T.stop(); return rc; }
    front_span(V.F);
    hipLaunchKernelGGL(dp_select, dim3(blocks_of(n)), dim3(256), 0, st, V);
    front_cut(V.F, V.keep, V.c_op);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    if (lra_exclusive_scan<uint32_t>(ctx, (long)n, c_op.p, op_off.p)) return fail(LRA_ERR_HIP, "lra_bam_depth: a scan failed");
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&n_op, op_off.p + n, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    S.ms_frame_select += T.stop();
  }
  {
    Timer T(st);
    if (!(grab(oplen, n_op + 1) && grab(ostart, n_op + 1))) return fail(LRA_ERR_NOMEM, "lra_bam_depth: hipMalloc failed for %llu CIGAR ops", (unsigned long long)n_op);
    V.oplen = oplen.p; V.ostart = ostart.p; V.n_op = n_op;
    if (n_op) hipLaunchKernelGGL(dp_oplen, dim3(blocks_of(n_op)), dim3(256), 0, st, V);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    if (lra_exclusive_scan<uint32_t>(ctx, (long)n_op, oplen.p, ostart.p)) return fail(LRA_ERR_HIP, "lra_bam_depth: a scan failed");
    hipLaunchKernelGGL(dp_ends, dim3(blocks_of(n)), dim3(256), 0, st, V);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    // what the plan needs of every record: keep u32 | ref i32 | pos i32 | end i64
    if (!h_meta.ensure(20 * n + 64, 0, st)) return fail(LRA_ERR_NOMEM, "lra_bam_depth: hipHostMalloc failed for the plan of %llu records", (unsigned long long)n);
    int64_t* h_end = (int64_t*)h_meta.p; uint32_t* h_keep = (uint32_t*)(h_end + n); int32_t* h_ref = (int32_t*)(h_keep + n); int32_t* h_pos = h_ref + n;
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(h_end, r_end.p, 8 * n, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(h_keep, keep.p, 4 * n, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(h_ref, r_ref.p, 4 * n, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(h_pos, r_pos.p, 4 * n, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(res, V.F.bad, sizeof res, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    S.ms_ops += T.stop();
    *stop_idx = res[B_STOP];
    const uint64_t lim = std::min<uint64_t>(n, res[B_STOP]);   // (what stands behind the region's end is not this pass's to refuse)
    uint64_t b = NONE; int kind = 0;
    for (int k : {B_ORDER, B_AUX, B_OP}) if (res[k] < lim && res[k] < b) { b = res[k]; kind = k; }   // (the lowest record; of two kinds at one record, the first)
    if (kind == B_ORDER) return refuse(b, "sorts in front of its predecessor: the file is not coordinate-sorted at " + where(b), bad_idx, bad_pos, bad_why);
    if (kind == B_AUX) return refuse(b, "has an aux block that ends inside a tag or names an unknown type", bad_idx, bad_pos, bad_why);
    if (kind == B_OP) return refuse(b, "has a CIGAR op code above 8", bad_idx, bad_pos, bad_why);
    // the plan: finish what lies below the next record, slide or grow when it reaches beyond the array, take the records that fit, and again
    std::vector<uint64_t> h_opoff;                             // (the op ranges of the prefixes: read where a prefix ends)
    const uint64_t n_take = lim;
    uint64_t kept = 0, i = 0;
    std::vector<std::pair<uint64_t, uint64_t>> segs;           // record ranges, in task order
    while (i < n_take) {
      if (!h_keep[i]) { i++; continue; }
      const int32_t r = h_ref[i];
      if (r != pl_ref) { plan_until_ref(w_tasks, r); plan_newref(w_tasks, r); }
      const int64_t lo = range_lo(r), hi = range_hi(r);
      const int64_t s = std::min(std::max<int64_t>(h_pos[i], lo), hi), e = std::min(std::max<int64_t>(h_end[i], lo), hi);
      if (e <= s) { kept++; i++; continue; }                    // nothing of it counts
      if (s > pl_base) { w_tasks.push_back(Task{T_FINISH, s, 0, 0}); pl_base = s; }
      if (e > pl_dbase + (int64_t)pl_span) {                     // beyond the array: it slides to the base, and doubles for a record longer than it
        while (e > pl_base + (int64_t)pl_span) pl_span *= 2;
        w_tasks.push_back(Task{T_SLIDE, (int64_t)pl_span, 0, 0}); pl_dbase = pl_base;
      }
      const uint64_t i0 = i;
      int64_t top = pl_live;
      while (i < n_take) {
        if (h_keep[i]) {
          if (h_ref[i] != r) break;
          const int64_t e2 = std::min(std::max<int64_t>(h_end[i], lo), hi);
          if (e2 > pl_dbase + (int64_t)pl_span) break;
          top = std::max(top, e2 + 1); kept++;
          pl_last = std::min(std::max<int64_t>(h_pos[i], lo), hi);
        }
        i++;
      }
      pl_live = top;
      segs.push_back({i0, i});
      w_tasks.push_back(Task{T_ACCUM, (int64_t)i0, (int64_t)i, top});
    }
    // the record ranges become op ranges
    if (!segs.empty()) {
      std::vector<uint64_t> edge(2 * segs.size());
      for (size_t k = 0; k < segs.size(); k++) {
        LRA_HIP_CHECK(ctx, hipMemcpyAsync(&edge[2 * k], op_off.p + segs[k].first, 8, hipMemcpyDeviceToHost, st));
        LRA_HIP_CHECK(ctx, hipMemcpyAsync(&edge[2 * k + 1], op_off.p + segs[k].second, 8, hipMemcpyDeviceToHost, st));
      }
      LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
      size_t k = 0;
      for (Task& t : w_tasks) if (t.kind == T_ACCUM) { t.a = (int64_t)edge[2 * k]; t.b = (int64_t)edge[2 * k + 1]; k++; }
    }
    w_have = true; w_ref = (uint32_t)h_ref[n - 1]; w_pos = h_pos[n - 1]; w_n = n; w_kept = kept;
  }
  return LRA_OK;
}

// One piece of the positions [base, to) of the reference in hand; *made: it is there to deliver.
int lra_bam_depth::finish_piece(int64_t to, struct lra_bam_depth_piece* piece, bool* made) {
  hipStream_t st = ctx->stream;
  *made = false;
  const bool zeros = base >= live;
  if (zeros && !prints_zeros()) { base = to; return LRA_OK; }  // nothing reaches these positions: the base jumps
  const int64_t hi = range_hi(cur_ref), b0 = range_lo(cur_ref);
  uint64_t m = (uint64_t)(to - base);
  if (!zeros) m = std::min<uint64_t>(m, (uint64_t)(live - base));
  const uint64_t per = std::max<uint64_t>(1, std::min(PIECE_POS, PIECE_TEXT / max_line));   // positions or bins of a piece
  Fin F; memset(&F, 0, sizeof F);
  F.first = base; F.ref = cur_ref; F.all = (int)O.all_positions; F.rname = (const char*)rname.p; F.rname_off = rname_off.p; F.carry = carry;
  F.red = (unsigned long long*)(misc.p + MISC_CNT);
  if (O.bin) m = std::min<uint64_t>(m, zeros ? per * O.bin : std::min<uint64_t>(PIECE_POS, per * O.bin)); else m = std::min(m, per);
  F.m = m;
  {
    Timer T(st);
    if (!zeros) {
      if (!(grab(doff, m + 1) && grab(depth, m))) return fail(LRA_ERR_NOMEM, "lra_bam_depth: hipMalloc failed for a piece of %llu positions", (unsigned long long)m);
      F.diff = dbuf[dcur].p + (base - dbase); F.depth = depth.p; F.off = doff.p;
      if (lra_exclusive_scan<int32_t>(ctx, (long)m, F.diff, doff.p)) return fail(LRA_ERR_HIP, "lra_bam_depth: a scan failed");
      hipLaunchKernelGGL(dp_depth, dim3(std::min(blocks_of(m), (unsigned)ctx->num_cu * 4u)), dim3(256), 0, st, F);
      LRA_HIP_CHECK(ctx, hipGetLastError());
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(&carry, depth.p + (m - 1), 4, hipMemcpyDeviceToHost, st));
    }
    uint64_t nb = 0;
    if (O.bin) {
      F.b0 = b0; F.range_end = hi; F.bin = O.bin; F.part = bin_part;
      F.k0 = (uint64_t)(base - b0) / O.bin;
      nb = (uint64_t)(base + (int64_t)m - 1 - b0) / O.bin - F.k0 + 1;
      F.nb = nb;
      if (!grab(sum, nb)) return fail(LRA_ERR_NOMEM, "lra_bam_depth: hipMalloc failed for %llu bins", (unsigned long long)nb);
      F.sum = sum.p;
      if (!zeros) {
        if (!grab(psum, m + 1)) return fail(LRA_ERR_NOMEM, "lra_bam_depth: hipMalloc failed for a piece of %llu positions", (unsigned long long)m);
        if (lra_exclusive_scan<uint32_t>(ctx, (long)m, depth.p, psum.p)) return fail(LRA_ERR_HIP, "lra_bam_depth: a scan failed");
        F.psum = psum.p;
      }
      hipLaunchKernelGGL(dp_bins, dim3(blocks_of(nb)), dim3(256), 0, st, F);
      LRA_HIP_CHECK(ctx, hipGetLastError());
      if (!h_sum.ensure(nb + 1, 0, st)) return fail(LRA_ERR_NOMEM, "lra_bam_depth: hipHostMalloc failed for %llu bins", (unsigned long long)nb);
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(h_sum.p, sum.p, 8 * nb, hipMemcpyDeviceToHost, st));
    }
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    S.ms_finish += T.stop();
    base += (int64_t)m;
    if (O.bin) {                                               // the bin the piece cuts waits for the next piece
      const int64_t last_end = std::min(b0 + (int64_t)((F.k0 + nb) * O.bin), hi);
      if (last_end > base) { bin_part = h_sum.p[nb - 1]; nb--; } else bin_part = 0;
      F.nb = nb;
    }
  }
  const uint64_t lanes = O.bin ? F.nb : m;
  uint64_t tlen = 0;
  if (O.want_text && lanes) {
    Timer T(st);
    if (!(grab(llen, lanes) && grab(loff, lanes + 1))) return fail(LRA_ERR_NOMEM, "lra_bam_depth: hipMalloc failed for the lines of a piece");
    F.llen = llen.p; F.loff = loff.p;
    if (O.bin) hipLaunchKernelGGL(dp_binlen, dim3(blocks_of(lanes)), dim3(256), 0, st, F); else hipLaunchKernelGGL(dp_linelen, dim3(blocks_of(lanes)), dim3(256), 0, st, F);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    if (lra_exclusive_scan<uint32_t>(ctx, (long)lanes, llen.p, loff.p)) return fail(LRA_ERR_HIP, "lra_bam_depth: a scan failed");
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&tlen, loff.p + lanes, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (tlen) {
      if (!grab(text, tlen + 64)) return fail(LRA_ERR_NOMEM, "lra_bam_depth: hipMalloc of %llu bytes for a piece's text failed", (unsigned long long)tlen);
      F.text = text.p;
      if (O.bin) hipLaunchKernelGGL(dp_binlines, dim3(blocks_of(lanes)), dim3(256), 0, st, F); else hipLaunchKernelGGL(dp_lines, dim3(blocks_of(lanes)), dim3(256), 0, st, F);
      LRA_HIP_CHECK(ctx, hipGetLastError());
    }
    S.ms_text += T.stop();
  }
  {
    Timer T(st);
    if (tlen) {
      if (!h_text.ensure(tlen + 1, 0, st)) return fail(LRA_ERR_NOMEM, "lra_bam_depth: hipHostMalloc of %llu bytes for a piece's text failed", (unsigned long long)tlen);
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(h_text.p, text.p, tlen, hipMemcpyDeviceToHost, st));
    }
    if (O.want_values && !O.bin) {
      if (!h_depth.ensure(m + 1, 0, st)) return fail(LRA_ERR_NOMEM, "lra_bam_depth: hipHostMalloc failed for a piece of %llu positions", (unsigned long long)m);
      if (zeros) memset(h_depth.p, 0, 4 * m); else LRA_HIP_CHECK(ctx, hipMemcpyAsync(h_depth.p, depth.p, 4 * m, hipMemcpyDeviceToHost, st));
    }
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    S.ms_copy += T.stop();
  }
  if (!lanes || (!tlen && !O.want_values)) return LRA_OK;
  piece->ref_id = cur_ref; piece->count = lanes; piece->text_len = tlen; piece->text = tlen ? h_text.p : nullptr;
  if (O.bin) { piece->first = b0 + (int64_t)(F.k0 * O.bin); piece->sum = O.want_values ? h_sum.p : nullptr; }
  else { piece->first = F.first; piece->depth = O.want_values ? h_depth.p : nullptr; }
  S.bytes_delivered += tlen + (O.want_values ? lanes * (O.bin ? 8 : 4) : 0);
  *made = true;
  return LRA_OK;
}

int lra_bam_depth::run_task(struct lra_bam_depth_piece* piece, bool* made) {
  hipStream_t st = ctx->stream;
  *made = false;
  Task& t = tasks.front();
  switch (t.kind) {
    case T_NEWREF:
      cur_ref = (int32_t)t.a; base = dbase = live = range_lo(cur_ref); carry = 0; bin_part = 0;
      tasks.pop_front();
      return LRA_OK;
    case T_FINISH:
      if (base >= t.a) { tasks.pop_front(); return LRA_OK; }
      return finish_piece(t.a, piece, made);
    case T_SLIDE: {
      const uint64_t cells = (uint64_t)t.a + 2, n_live = live > base ? (uint64_t)(live - base) : 0;
      Timer T(st);
      if (n_live || span != (uint64_t)t.a) {
        Buf<int32_t>& dst = dbuf[dcur ^ 1];
        if (dst.n < cells) {
          if (!grab(dst, cells)) return fail(LRA_ERR_NOMEM, "lra_bam_depth: hipMalloc failed for a position window of %llu bases", (unsigned long long)t.a);
          LRA_HIP_CHECK(ctx, hipMemsetAsync(dst.p, 0, dst.n * sizeof(int32_t), st));
        }
        if (n_live) hipLaunchKernelGGL(dp_slide, dim3(blocks_of(n_live)), dim3(256), 0, st, dst.p, dbuf[dcur].p, (uint64_t)(base - dbase), n_live);
        LRA_HIP_CHECK(ctx, hipGetLastError());
        dcur ^= 1;
      }
      span = (uint64_t)t.a; dbase = base; S.slides++;
      S.ms_accumulate += T.stop();
      tasks.pop_front();
      return LRA_OK;
    }
    default: {
      Timer T(st);
      Acc A; A.diff = dbuf[dcur].p; A.dbase = dbase; A.cells = std::min<uint64_t>(span + 1, dbuf[dcur].n); A.lo_c = range_lo(cur_ref); A.hi_c = range_hi(cur_ref);
      A.o_lo = (uint64_t)t.a; A.o_hi = (uint64_t)t.b; A.outside = (unsigned int*)(misc.p + MISC_CNT + 3);
      if (A.o_hi > A.o_lo) {
        hipLaunchKernelGGL(dp_accum, dim3(blocks_of(A.o_hi - A.o_lo)), dim3(256), 0, st, V, A);
        LRA_HIP_CHECK(ctx, hipGetLastError());
        dirty = true;
      }
      live = std::max(live, t.c);
      S.ms_accumulate += T.stop();
      tasks.pop_front();
      return LRA_OK;
    }
  }
}

int lra_bam_depth::next(struct lra_bam_depth_piece* piece) {
  hipStream_t st = ctx->stream;
  memset(piece, 0, sizeof *piece);
  for (;;) {
    while (!tasks.empty()) {
      bool made = false;
      if (int rc = run_task(piece, &made)) { tasks.clear(); done = true; return rc; }
      if (made) return LRA_OK;
    }
    if (done && !flushed) return LRA_OK;
    if (flushed) {                                             // the pass is over and everything is out: the stats' reductions come back
      unsigned long long red[4] = {0, 0, 0, 0};
      if (misc.p) {
        LRA_HIP_CHECK(ctx, hipMemcpyAsync(red, misc.p + MISC_CNT, 32, hipMemcpyDeviceToHost, st));
        LRA_HIP_CHECK(ctx, hipMemsetAsync(misc.p + MISC_CNT, 0, 32, st));
        LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
        S.covered += red[0]; S.depth_sum += red[1]; S.depth_max = std::max<uint64_t>(S.depth_max, red[2]);
        if ((unsigned int)red[3]) return fail(LRA_ERR_HIP, "lra_bam_depth: %u adds fell outside the position window", (unsigned int)red[3]);
      }
      flushed = false; dirty = false;
      return LRA_OK;
    }
    int state = 0;
    if (int rc = step(*this, &state)) { tasks.clear(); done = true; return rc; }
    if (state == 2) {                                          // every record is in: the rest of the range is final
      std::vector<Task> t;
      if (mode == 2) plan_until_ref(t, ref_id + 1); else if (mode == 1) plan_until_ref(t, refs.n_ref);
      for (const Task& x : t) tasks.push_back(x);
      flushed = done = true;
    }
  }
}

extern "C" int lra_bam_depth_create(lra_ctx* ctx, const char* bam_path, const char* bai_path, const struct lra_bam_depth_opts* opts, lra_bam_depth** out) {
  if (!ctx || !bam_path || !out) return LRA_ERR_INVALID;
  *out = nullptr;
  std::unique_ptr<lra_bam_depth> d(new lra_bam_depth());
  if (opts) d->O = *opts; else { d->O.exclude = ~0u; d->O.want_text = 1; }
  if (d->O.exclude == ~0u) d->O.exclude = DEFAULT_EXCLUDE;
  if (!d->O.want_text && !d->O.want_values) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_bam_depth_create: neither text nor values are wanted");
  d->span = d->O.span_bases ? std::max(d->O.span_bases, MIN_SPAN) : DEFAULT_SPAN;
  if (int rc = d->open_files(ctx, "lra_bam_depth", bam_path, bai_path, d->O.window_bytes)) return pass_create_failed(d.get(), rc);
  uint64_t longest = 1;
  for (const std::string& s : d->refs.name) longest = std::max<uint64_t>(longest, s.size());
  d->max_line = longest + 48;                                  // a name, three numbers of at most 10, 10 and 23 bytes, the separators
  // misc behind the pass's words: the stats' reductions [MISC_CNT, MISC_CNT + 3), the adds outside the array [MISC_CNT + 3]
  if (!d->zero_misc()) return pass_create_failed(d.get(), lra_set_err(ctx, LRA_ERR_NOMEM, "lra_bam_depth_create: hipMalloc failed"));
  *out = d.release();
  return LRA_OK;
}

extern "C" void lra_bam_depth_destroy(lra_bam_depth* d) { pass_destroy(d); }

extern "C" int lra_bam_depth_header(lra_bam_depth* d, int* n_ref, const char* const** names, const uint64_t** ref_len) {
  return d ? d->header_refs(n_ref, names, ref_len) : LRA_ERR_INVALID;
}

extern "C" int lra_bam_depth_all(lra_bam_depth* d) {
  if (!d) return LRA_ERR_INVALID;
  d->tasks.clear(); d->flushed = false; d->done = true;
  if (int rc = d->pass_all()) return rc;
  return d->begin_pass();
}

extern "C" int lra_bam_depth_region(lra_bam_depth* d, int32_t ref_id, int64_t beg, int64_t end) {
  if (!d) return LRA_ERR_INVALID;
  d->tasks.clear(); d->flushed = false; d->done = true;
  if (int rc = d->pass_region(ref_id, beg, end)) return rc;
  return d->begin_pass();
}

extern "C" int lra_bam_depth_next(lra_bam_depth* d, struct lra_bam_depth_piece* piece) {
  if (!d || !piece) return LRA_ERR_INVALID;
  LRA_HIP_CHECK(d->ctx, hipSetDevice(d->ctx->device));
  return d->next(piece);
}

extern "C" int lra_bam_depth_stats(lra_bam_depth* d, struct lra_bam_depth_stats* out) {
  if (!d || !out) return LRA_ERR_INVALID;
  *out = d->S;
  d->add_stats(out);
  return LRA_OK;
}

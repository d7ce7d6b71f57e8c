// lra_amd/csrc/bam_svcalls.hip -- lra_bam_svcalls: the merged DEL and INS tables of one haplotype's assembly alignments, from a coordinate-sorted BAM (gfx950).
// The one-haplotype half of the reference's call_assembly_SVs snakefile -- parseAlignment, CallSV, FilterBySizeAndSVTYPE, FilterByCentromereAndAltChromAndAddID,
// mergeCalls -- with the variant table on the device from the records to the printed lines.  include/lra_hip.h has the interface and the rules; bam_pass.h is
// the pass, bam_contained.h the filter, bam_vcf_walk.h the walk (all shared with lra_bam_vcf); bam_svcalls_host.h the arithmetic host and kernels share.
//
// window.  sv_order, a lane per record: (refID, pos) against the record in front (the carried key for the first), refID -1 last -- the filter and the
// delivery by reference rely on the order.  The walk (min_length = min_size, the runs that fail it counted) leaves the window's variants.  sv_flag, a lane per
// variant: the mask test, a flag per kind.  Two scans number the survivors: NR = the pass's count of the kind + the scan + 1.  sv_rows writes a row per
// survivor behind the kind's table; one scan of l_name + alt_len places what the table keeps of the window -- QNAME and ALT, which cannot be had again --
// and sv_bytes, a wave per row, copies them (ALT through wave_seq).  REF is not kept: the genome is resident.  Nothing of this is the pass's until the window
// is delivered: a window run again in front of a refused record writes the same tail again.
// reference.  A reference is final when a record of a later one has been delivered or the pass ends.  Its rows are the table's head (the file is sorted).
// sv_tiles: the interval every 256 rows in NR order lie in.  sv_deg, a lane per row i: the rows k < i with R(k, i) -- whole tiles whose interval shares no
// base with row i passed over -- counted, then (one scan) written as row i's in-edges by sv_fill.  sv_round: a row is kept once every
// in-neighbour is dropped and dropped once one is kept, from the states the round before left (two arrays, so the rounds do not depend on the lanes' order);
// eight rounds per read-back, until a round decides nothing.  NR order is nearly position order (the file is sorted; a record's variants ascend), so a
// tile's interval is narrow and a row tests the tiles near it: M / 256 interval tests a row and the rows of the tiles it meets, quadratic only where every
// row meets every tile.  sv_kept, one scan, sv_plen: the kept rows in NR order and their lines' four pieces
//   RNAME \t START \t [END \t] ID \t | REF | \t ALT | \t 60 \t PASS \t SVTYPE= .. QSTRAND= . \t GT \t 1/1 \n
// sv_small prints the first and the last and the value record, sv_bulk (chunk_copy.h's walk) copies REF from the genome and ALT from the kept bytes.
// sv_pop moves the rows behind the head, and their bytes, to the front.
// sink (bam_sv_table.h; lra_sv_combine's, no part of the ABI).  With one set, the kept rows are not printed: sv_sink_len, one scan and sv_sink_copy, a wave
// per kept row, append them and their bytes to the sink's table of the kind, b_off rebased, in front of sv_pop.  Without one nothing here differs.
#include "common.h"
#include "chunk_copy.h"
#include "scan.h"
#include "bam_pass.h"
#include "bam_vcf_walk.h"
#include "bam_sv_table.h"
#include "bam_svcalls_host.h"
#include <stddef.h>
#include <algorithm>
#include <string>
#include <vector>

namespace {

constexpr int SV_BATCH = 8, SV_TILE = 256;
enum { M_UNSORTED = 0, M_LAST = 1, M_HAS_LAST = 2, M_MASKED_INS = 3, M_MASKED_DEL = 4, M_PREFIX = 5, M_BASE = 6, M_CHANGED = 8, M_WORDS = 16 };   // sv_misc[]

// ---- the window ------------------------------------------------------------------------------------------------------------------------------------------------
struct SvW {
  const uint8_t* data; const uint64_t* pos; uint64_t n, limit; int region;
  unsigned long long* misc;
  const Var* var; uint64_t nv, ord_base;
  const uint64_t* moff; const int64_t* mbeg; const int64_t* mend;
  uint32_t* flag[2]; uint64_t* foff[2];                       // [0] INS, [1] DEL
  SvRow* rows[2]; uint64_t nr_base[2];                        // the tables' tails
  uint32_t* src[2]; uint32_t* blen[2]; uint64_t* boff[2]; uint8_t* bytes[2]; uint64_t bbase[2]; uint64_t count[2];
};

__global__ void __launch_bounds__(256) sv_order(SvW W, unsigned long long last, int has_last) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= W.n) return;
  const uint64_t at = W.pos[i];
  if (W.region && at >= W.limit) return;                       // (the next chunk reads it again)
  const uint8_t* p = W.data + at;
  const unsigned long long key = ((unsigned long long)le32(p + 4) << 32) | (uint32_t)((int32_t)le32(p + 8) + 0x80000000u);   // refID -1 is the largest; pos in order as unsigned
  unsigned long long prev = last; bool has = has_last != 0;
  if (i) { const uint8_t* q = W.data + W.pos[i - 1]; prev = ((unsigned long long)le32(q + 4) << 32) | (uint32_t)((int32_t)le32(q + 8) + 0x80000000u); has = true; }
  if (has && key < prev) atomicMin(&W.misc[M_UNSORTED], (unsigned long long)i);
  if (i + 1 == W.n || (W.region && W.pos[i + 1] >= W.limit)) { W.misc[M_LAST] = key; W.misc[M_HAS_LAST] = 1; }   // (one lane: the positions ascend)
}

__global__ void __launch_bounds__(256) sv_flag(SvW W) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool mi = false, md = false;
  if (j < W.nv) {
    const Var& v = W.var[j];
    const int64_t start = v.anchor, stop = start + (v.svlen < 0 ? -v.svlen : v.svlen);
    const bool masked = lra_sv_masked(W.mbeg, W.mend, W.moff[v.ref], W.moff[v.ref + 1], start, stop);
    W.flag[0][j] = !v.del && !masked ? 1u : 0u; W.flag[1][j] = v.del && !masked ? 1u : 0u;
    mi = masked && !v.del; md = masked && v.del;
  }
  const unsigned long long bi = __ballot(mi), bd = __ballot(md);
  if ((threadIdx.x & 63) == 0) {
    if (bi) atomicAdd(&W.misc[M_MASKED_INS], (unsigned long long)__popcll(bi));
    if (bd) atomicAdd(&W.misc[M_MASKED_DEL], (unsigned long long)__popcll(bd));
  }
}

__global__ void __launch_bounds__(256) sv_rows(SvW W) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= W.nv) return;
  const Var& v = W.var[j];
  const int k = v.del ? 1 : 0;
  if (!W.flag[k][j]) return;
  const uint64_t i = W.foff[k][j];
  SvRow r;
  r.start = v.anchor; r.end = r.start + (v.svlen < 0 ? -v.svlen : v.svlen); r.svlen = v.svlen; r.nr = W.nr_base[k] + i + 1; r.record = W.ord_base + v.rec;
  r.g_at = v.g_at; r.ref_len = v.ref_len; r.alt_len = v.alt_len; r.b_off = 0; r.ref = v.ref; r.qstart = (uint32_t)(v.aq + 1); r.l_name = v.l_name; r.reverse = (v.flag & 16u) ? 1u : 0u;
  W.rows[k][i] = r;
  W.src[k][i] = (uint32_t)j; W.blen[k][i] = v.l_name + (uint32_t)v.alt_len;   // (alt_len <= l_seq, a record's bytes: below 2^32 with the name)
}

// a wave per row of kind k: QNAME, then ALT decoded
__global__ void __launch_bounds__(256) sv_bytes(SvW W, int k) {
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const int lane = threadIdx.x & 63;
  for (uint64_t i = wave; i < W.count[k]; i += n_waves) {
    const Var& v = W.var[W.src[k][i]];
    const uint64_t at = W.bbase[k] + W.boff[k][i];
    uint8_t* d = W.bytes[k] + at;
    for (uint32_t c = lane; c < v.l_name; c += 64) d[c] = W.data[v.name_at + c];
    wave_seq(d + v.l_name, W.data + v.seq_at, v.aq, v.alt_len, lane);
    if (lane == 0) W.rows[k][i].b_off = at;
  }
}

// ---- a reference's rows of one kind (SvF and the line emitter: bam_sv_table.h) -----------------------------------------------------------------------------------
// rows [0, n) are sorted by reference: how many lie at or below r
__global__ void __launch_bounds__(256) sv_prefix(const SvRow* rows, uint64_t n, int32_t r, unsigned long long* out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (rows[i].ref <= r && (i + 1 == n || rows[i + 1].ref > r)) *out = i + 1;   // (one lane at most; the host has zeroed *out)
}

// a block per tile of rows: the interval the tile's rows lie in.  A row shares a base with none of them unless it shares one with that interval.
__global__ void __launch_bounds__(SV_TILE) sv_tiles(SvF F) {
  __shared__ int64_t lo[SV_TILE / 64], hi[SV_TILE / 64];
  const uint64_t i = (uint64_t)blockIdx.x * SV_TILE + threadIdx.x;
  int64_t a = i < F.m ? F.rows[i].start : INT64_MAX, b = i < F.m ? F.rows[i].end : INT64_MIN;
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t a2 = (int64_t)__shfl_xor((unsigned long long)a, o), b2 = (int64_t)__shfl_xor((unsigned long long)b, o);
    a = a2 < a ? a2 : a; b = b2 > b ? b2 : b;
  }
  if ((threadIdx.x & 63) == 0) { lo[threadIdx.x >> 6] = a; hi[threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < SV_TILE / 64; w++) { a = lo[w] < a ? lo[w] : a; b = hi[w] > b ? hi[w] : b; }
    F.t_lo[blockIdx.x] = a; F.t_hi[blockIdx.x] = b;
  }
}
// the rows k < i with R(k, i), in ascending k: f(k) for each.  Whole tiles whose interval shares no base with row i are passed over (ov > 0 needs one).
template <typename Fn> __device__ __forceinline__ void sv_earlier_related(const SvF& F, uint64_t i, Fn f) {
  const int64_t s = F.rows[i].start, e = F.rows[i].end;
  for (uint64_t t = 0; t * SV_TILE < i; t++) {
    if (F.t_lo[t] >= e || F.t_hi[t] <= s) continue;
    const uint64_t k1 = min((t + 1) * (uint64_t)SV_TILE, i);
    for (uint64_t k = t * SV_TILE; k < k1; k++) if (lra_sv_related(F.rows[k].start, F.rows[k].end, s, e)) f(k);
  }
}
__global__ void __launch_bounds__(256) sv_deg(SvF F) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= F.m) return;
  uint32_t d = 0;
  sv_earlier_related(F, i, [&](uint64_t) { d++; });
  F.deg[i] = d;
}
__global__ void __launch_bounds__(256) sv_fill(SvF F) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= F.m) return;
  uint64_t at = F.eoff[i];
  if (at == F.eoff[i + 1]) return;
  sv_earlier_related(F, i, [&](uint64_t k) { F.in[at++] = (uint32_t)k; });
}
__global__ void __launch_bounds__(256) sv_round(SvF F, const uint32_t* a, uint32_t* b, unsigned long long* changed) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool ch = false;
  if (i < F.m) {
    const uint32_t was = a[i];
    const uint32_t now = was != LRA_SV_OPEN ? was : lra_sv_decide(a, F.in, F.eoff[i], F.eoff[i + 1]);
    b[i] = now; ch = now != was;
  }
  if (__ballot(ch) && (threadIdx.x & 63) == 0) *changed = 1;
}
__global__ void __launch_bounds__(256) sv_kept(SvF F, const uint32_t* state) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < F.m) F.kept[i] = state[i] == LRA_SV_KEPT ? 1u : 0u;
}
// ---- the sink: the kept rows of a reference, appended to another object's table ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) sv_sink_len(SvF F, uint32_t* blen) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= F.nk) return;
  const SvRow& r = F.rows[F.kidx[j]];
  blen[j] = r.l_name + (uint32_t)r.alt_len;
}
// a wave per kept row: the row behind out[0, at_row) with b_off rebased, its bytes behind out_bytes[0, at_byte)
__global__ void __launch_bounds__(256) sv_sink_copy(SvF F, const uint64_t* boff, SvRow* out, uint64_t at_row, uint8_t* out_bytes, uint64_t at_byte) {
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const int lane = threadIdx.x & 63;
  for (uint64_t j = wave; j < F.nk; j += n_waves) {
    const SvRow& r = F.rows[F.kidx[j]];
    const uint64_t to = at_byte + boff[j], n = (uint64_t)r.l_name + r.alt_len;
    for (uint64_t c = lane; c < n; c += 64) out_bytes[to + c] = F.bytes[r.b_off + c];
    if (lane == 0) { SvRow* o = out + at_row + j; *o = r; o->b_off = to; }
  }
}

// the rows [from, n) move to the front of `out`, their bytes' offsets less the first one's (*base, for the host's copy of the bytes)
__global__ void __launch_bounds__(256) sv_pop(const SvRow* rows, SvRow* out, uint64_t from, uint64_t n, unsigned long long* base) {
  const uint64_t i = from + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t b = rows[from].b_off;                         // (the bytes were appended in row order)
  SvRow r = rows[i]; r.b_off -= b;
  out[i - from] = r;
  if (i == from) *base = b;
}

}  // namespace

struct lra_bam_svcalls : lra_bam_pass {
  lra_bam_svcalls_opts O{}; lra_vcf_rules rules{}; std::string stem[2];
  const unsigned char* d_genome = nullptr; const uint64_t* d_chrom_pos = nullptr;
  struct lra_bam_svcalls_stats S{};
  lra_vcf_walk W;
  // the mask, as the kernels search it
  Buf<uint64_t> moff; Buf<int64_t> mbeg, mend; Buf<char> d_stem[2];
  // the window
  Buf<unsigned long long> sv_misc; Buf<uint32_t> flag[2], src[2], blen[2]; Buf<uint64_t> foff[2], boff[2];
  uint64_t w_n = 0, w_cnt[N_CNT] = {}, w_rows[2] = {0, 0}, w_bytes[2] = {0, 0}, w_masked[2] = {0, 0}; unsigned long long w_last = 0; bool w_has_last = false;
  // the pass: the tables ([0] INS, [1] DEL), two of each so that sv_pop has somewhere to move to
  KeepBuf<SvRow> rows[2][2]; KeepBuf<uint8_t> bytes[2][2]; int cur[2] = {0, 0};
  uint64_t n_rows[2] = {0, 0}, n_bytes[2] = {0, 0}, nr_base[2] = {0, 0}, pass_recs = 0;
  unsigned long long last_key = 0; bool has_last = false, faulted = false;
  int32_t fin_ref = -1; int fin_stage = 0; uint64_t fin_m[2] = {0, 0};   // the reference being delivered: stage 0 none, 1 its DEL piece is next, 2 its INS piece, 3 the pop
  // a reference's rows
  Buf<uint32_t> deg, in, st_a, st_b, kept, kidx, plen; Buf<uint64_t> eoff, koff, poff; Buf<int64_t> t_lo, t_hi; Buf<uint8_t> text; Buf<struct lra_bam_svcalls_row> vals;
  PinBuf<char> h_text; PinBuf<struct lra_bam_svcalls_row> h_vals;
  lra_sv_sink* sink = nullptr; Buf<uint32_t> s_len; Buf<uint64_t> s_off;   // set: a reference's kept rows go there and nothing is printed

  lra_bam_svcalls() { W.ms_frame_select = &S.ms_frame_select; W.ms_ops = &S.ms_ops; W.ms_walk = &S.ms_walk; W.ms_lengths = &S.ms_lengths; }
  void release_all() {
    release_pass(); W.release(); moff.release(); mbeg.release(); mend.release(); sv_misc.release();
    for (int k = 0; k < 2; k++) {
      d_stem[k].release(); flag[k].release(); src[k].release(); blen[k].release(); foff[k].release(); boff[k].release();
      for (int b = 0; b < 2; b++) { rows[k][b].release(); bytes[k][b].release(); }
    }
    t_lo.release(); t_hi.release(); deg.release(); in.release(); st_a.release(); st_b.release(); kept.release(); kidx.release(); plen.release(); eoff.release(); koff.release(); poff.release(); text.release(); vals.release();
    h_text.release(); h_vals.release(); s_len.release(); s_off.release();
  }
  int take_genome(const char* fn) { return lra_vcf_take_genome(*this, fn, &d_genome, &d_chrom_pos); }
  int set_mask(uint64_t n, const int32_t* ref_id, const int64_t* b, const int64_t* e);
  int begin_pass() {
    pass_recs = 0; has_last = false; faulted = false; fin_stage = 0;
    for (int k = 0; k < 2; k++) n_rows[k] = n_bytes[k] = nr_base[k] = 0;
    forget();
    return W.begin(*this, O.drop_contained != 0);
  }
  // the pass's consumer
  int window(uint64_t n, uint64_t limit, uint64_t* bad_idx, uint64_t* bad_pos, std::string* bad_why, uint64_t* stop_idx);
  void forget() { w_n = 0; memset(w_cnt, 0, sizeof w_cnt); w_rows[0] = w_rows[1] = w_bytes[0] = w_bytes[1] = w_masked[0] = w_masked[1] = 0; w_has_last = false; W.forget(); }
  bool deliver() {
    S.records_read += w_n; S.records_walked += w_cnt[N_WALKED]; S.records_contained += w_cnt[N_CONTAINED];
    S.small_ins += w_cnt[N_SMALL_INS]; S.small_del += w_cnt[N_SMALL_DEL]; S.masked_ins += w_masked[0]; S.masked_del += w_masked[1];
    W.commit(*this);
    for (int k = 0; k < 2; k++) { n_rows[k] += w_rows[k]; n_bytes[k] += w_bytes[k]; nr_base[k] += w_rows[k]; }
    if (w_has_last) { last_key = w_last; has_last = true; }
    pass_recs += w_n;
    return false;                                              // (next() looks at the tables itself)
  }
  int finish_kind(int k, uint64_t m, struct lra_bam_svcalls_piece* piece);
  int to_sink(int k, SvF& F, uint64_t nk, struct lra_bam_svcalls_piece* piece);
  int pop(int k, uint64_t m);
  int next(struct lra_bam_svcalls_piece* piece);
};

int lra_bam_svcalls::set_mask(uint64_t n, const int32_t* ref_id, const int64_t* b, const int64_t* e) {
  lra_sv_mask m; std::string why;
  if (!lra_sv_mask_build(refs.n_ref, n, ref_id, b, e, &m, &why)) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_bam_svcalls_set_mask: %s", why.c_str());
  hipStream_t st = ctx->stream;
  if (!moff.ensure(m.off.size()) || !mbeg.ensure(m.beg.size() + 1) || !mend.ensure(m.end.size() + 1)) { (void)hipGetLastError(); return lra_set_err(ctx, LRA_ERR_NOMEM, "lra_bam_svcalls_set_mask: hipMalloc failed"); }
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  LRA_HIP_CHECK(ctx, hipMemcpy(moff.p, m.off.data(), 8 * m.off.size(), hipMemcpyHostToDevice));
  if (!m.beg.empty()) {
    LRA_HIP_CHECK(ctx, hipMemcpy(mbeg.p, m.beg.data(), 8 * m.beg.size(), hipMemcpyHostToDevice));
    LRA_HIP_CHECK(ctx, hipMemcpy(mend.p, m.end.data(), 8 * m.end.size(), hipMemcpyHostToDevice));
  }
  return LRA_OK;
}

int lra_bam_svcalls::window(uint64_t n, uint64_t limit, uint64_t* bad_idx, uint64_t* bad_pos, std::string* bad_why, uint64_t* stop_idx) {
  hipStream_t st = ctx->stream;
  *bad_idx = NONE; *stop_idx = NONE;
  forget();
  Vc V; memset(&V, 0, sizeof V);
  V.rules = rules; V.count_small = 1; V.genome = d_genome; V.chrom_pos = d_chrom_pos; V.ord_base = pass_recs;
  if (int rc = W.check(*this, V, n, limit, bad_idx, bad_pos, bad_why)) return rc;
  if (*bad_idx != NONE) return LRA_OK;
  SvW X; memset(&X, 0, sizeof X);
  X.data = z.data; X.pos = pos.p; X.n = n; X.limit = limit; X.region = mode == 2; X.misc = sv_misc.p;
  unsigned long long mres[M_WORDS];
  {
    Timer T(st);
    LRA_HIP_CHECK(ctx, hipMemsetAsync(sv_misc.p, 0, 8 * M_WORDS, st));
    LRA_HIP_CHECK(ctx, hipMemsetAsync(sv_misc.p + M_UNSORTED, 0xff, 8, st));
    hipLaunchKernelGGL(sv_order, dim3(blocks_of(n)), dim3(256), 0, st, X, last_key, has_last ? 1 : 0);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(mres, sv_misc.p, 8 * M_WORDS, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    S.ms_frame_select += T.stop();
  }
  if (mres[M_UNSORTED] < n)                                   // the records in front of it go first; what the walk refuses among them is refused then
    return refuse(mres[M_UNSORTED], "sorts in front of its predecessor: the file is not coordinate-sorted at " + where(mres[M_UNSORTED]), bad_idx, bad_pos, bad_why);
  uint64_t nv = 0, total = 0;
  if (int rc = W.walk(*this, V, O.drop_contained != 0, false, bad_idx, bad_pos, bad_why, stop_idx, &nv, &total, w_cnt)) return rc;
  if (*bad_idx != NONE) return LRA_OK;
  w_n = n; w_last = mres[M_LAST]; w_has_last = mres[M_HAS_LAST] != 0;
  if (!nv) return LRA_OK;
  Timer T(st);
  for (int k = 0; k < 2; k++)
    if (!grab(flag[k], nv) || !grab(foff[k], nv + 1)) return fail(LRA_ERR_NOMEM, "lra_bam_svcalls: hipMalloc failed for %llu variants", (unsigned long long)nv);
  X.var = W.var.p; X.nv = nv; X.ord_base = pass_recs; X.moff = moff.p; X.mbeg = mbeg.p; X.mend = mend.p;
  for (int k = 0; k < 2; k++) { X.flag[k] = flag[k].p; X.foff[k] = foff[k].p; X.nr_base[k] = nr_base[k]; }
  hipLaunchKernelGGL(sv_flag, dim3(blocks_of(nv)), dim3(256), 0, st, X);
  LRA_HIP_CHECK(ctx, hipGetLastError());
  uint64_t cnt[2] = {0, 0};
  for (int k = 0; k < 2; k++) {
    if (lra_exclusive_scan<uint32_t>(ctx, (long)nv, flag[k].p, foff[k].p)) return fail(LRA_ERR_HIP, "lra_bam_svcalls: a scan failed");
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&cnt[k], foff[k].p + nv, 8, hipMemcpyDeviceToHost, st));
  }
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(mres, sv_misc.p, 8 * M_WORDS, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  w_masked[0] = mres[M_MASKED_INS]; w_masked[1] = mres[M_MASKED_DEL];
  if (cnt[0] + cnt[1]) {
    for (int k = 0; k < 2; k++) {
      if (!rows[k][cur[k]].ensure(n_rows[k] + cnt[k], n_rows[k], st) || !grab(src[k], cnt[k]) || !grab(blen[k], cnt[k]) || !grab(boff[k], cnt[k] + 1))
        return fail(LRA_ERR_NOMEM, "lra_bam_svcalls: hipMalloc failed for %llu rows", (unsigned long long)(n_rows[k] + cnt[k]));
      X.rows[k] = rows[k][cur[k]].p + n_rows[k]; X.src[k] = src[k].p; X.blen[k] = blen[k].p; X.boff[k] = boff[k].p; X.count[k] = cnt[k]; X.bbase[k] = n_bytes[k];
    }
    hipLaunchKernelGGL(sv_rows, dim3(blocks_of(nv)), dim3(256), 0, st, X);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    uint64_t nb[2] = {0, 0};
    for (int k = 0; k < 2; k++) {
      if (lra_exclusive_scan<uint32_t>(ctx, (long)cnt[k], blen[k].p, boff[k].p)) return fail(LRA_ERR_HIP, "lra_bam_svcalls: a scan failed");
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(&nb[k], boff[k].p + cnt[k], 8, hipMemcpyDeviceToHost, st));
    }
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    for (int k = 0; k < 2; k++) {
      if (!cnt[k]) continue;
      if (!bytes[k][cur[k]].ensure(n_bytes[k] + nb[k] + 8, n_bytes[k], st)) return fail(LRA_ERR_NOMEM, "lra_bam_svcalls: hipMalloc of %llu bytes for the rows' names and ALT failed", (unsigned long long)(n_bytes[k] + nb[k]));
      X.bytes[k] = bytes[k][cur[k]].p;
      hipLaunchKernelGGL(sv_bytes, dim3(wave_blocks(ctx, cnt[k])), dim3(256), 0, st, X, k);
    }
    LRA_HIP_CHECK(ctx, hipGetLastError());
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    for (int k = 0; k < 2; k++) { w_rows[k] = cnt[k]; w_bytes[k] = nb[k]; }
  }
  S.ms_rows += T.stop();
  return LRA_OK;
}

// The rows [0, m) of kind k are one reference's, final: merged, and the kept ones printed into *piece.
int lra_bam_svcalls::finish_kind(int k, uint64_t m, struct lra_bam_svcalls_piece* piece) {
  hipStream_t st = ctx->stream;
  SvF F; memset(&F, 0, sizeof F);
  F.rows = rows[k][cur[k]].p; F.m = m; F.misc = sv_misc.p;
  uint64_t n_edge = 0, nk = 0, rounds = 0;
  {
    Timer T(st);
    const uint64_t n_tile = (m + SV_TILE - 1) / SV_TILE;
    if (!(grab(t_lo, n_tile) && grab(t_hi, n_tile) && grab(deg, m) && grab(eoff, m + 1) && grab(st_a, m) && grab(st_b, m) && grab(kept, m) && grab(koff, m + 1) && grab(kidx, m)))
      return fail(LRA_ERR_NOMEM, "lra_bam_svcalls: hipMalloc failed for the merge of %llu rows", (unsigned long long)m);
    F.t_lo = t_lo.p; F.t_hi = t_hi.p; F.deg = deg.p; F.eoff = eoff.p; F.st_a = st_a.p; F.st_b = st_b.p; F.kept = kept.p; F.koff = koff.p; F.kidx = kidx.p;
    hipLaunchKernelGGL(sv_tiles, dim3((unsigned)n_tile), dim3(SV_TILE), 0, st, F);
    hipLaunchKernelGGL(sv_deg, dim3(blocks_of(m)), dim3(256), 0, st, F);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    if (lra_exclusive_scan<uint32_t>(ctx, (long)m, deg.p, eoff.p)) return fail(LRA_ERR_HIP, "lra_bam_svcalls: a scan failed");
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&n_edge, eoff.p + m, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (!grab(in, n_edge + 1)) return fail(LRA_ERR_NOMEM, "lra_bam_svcalls: hipMalloc failed for %llu pairs of related rows", (unsigned long long)n_edge);
    F.in = in.p;
    if (n_edge) hipLaunchKernelGGL(sv_fill, dim3(blocks_of(m)), dim3(256), 0, st, F);
    LRA_HIP_CHECK(ctx, hipMemsetAsync(st_a.p, 0, 4 * m, st));
    uint32_t* a = st_a.p; uint32_t* b = st_b.p;
    for (bool done = false; !done;) {                           // SV_BATCH rounds, then one look at what they decided: a round that decides nothing ends the merge
      unsigned long long ch[SV_BATCH];
      LRA_HIP_CHECK(ctx, hipMemsetAsync(sv_misc.p + M_CHANGED, 0, 8 * SV_BATCH, st));
      for (int r = 0; r < SV_BATCH; r++) { hipLaunchKernelGGL(sv_round, dim3(blocks_of(m)), dim3(256), 0, st, F, a, b, sv_misc.p + M_CHANGED + r); std::swap(a, b); }
      LRA_HIP_CHECK(ctx, hipGetLastError());
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(ch, sv_misc.p + M_CHANGED, 8 * SV_BATCH, hipMemcpyDeviceToHost, st));
      LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
      for (int r = 0; r < SV_BATCH && !done; r++) { if (ch[r]) rounds++; else done = true; }
    }
    hipLaunchKernelGGL(sv_kept, dim3(blocks_of(m)), dim3(256), 0, st, F, (const uint32_t*)a);   // (a: the last round's output; the rounds behind the deciding ones copy it)
    LRA_HIP_CHECK(ctx, hipGetLastError());
    if (lra_exclusive_scan<uint32_t>(ctx, (long)m, kept.p, koff.p)) return fail(LRA_ERR_HIP, "lra_bam_svcalls: a scan failed");
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&nk, koff.p + m, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    S.ms_merge += T.stop();
  }
  S.merge_rounds += rounds;
  (k ? S.merged_del : S.merged_ins) += m - nk; (k ? S.kept_del : S.kept_ins) += nk;
  if (sink) return to_sink(k, F, nk, piece);
  uint64_t total = 0, dev_text = 0, host_text = 0, value_bytes = 0;
  {
    Timer T(st);
    if (O.want_text && !(grab(plen, 4 * nk) && grab(poff, 4 * nk + 1))) return fail(LRA_ERR_NOMEM, "lra_bam_svcalls: hipMalloc failed for %llu rows", (unsigned long long)nk);
    F.nk = nk; F.plen = O.want_text ? plen.p : nullptr; F.poff = poff.p;
    F.rname = (const char*)rname.p; F.rname_off = rname_off.p; F.genome = d_genome; F.bytes = bytes[k][cur[k]].p;
    F.stem = d_stem[k].p; F.stem_len = (uint32_t)stem[k].size(); F.del = k; F.one_based = O.pos_one_based ? 1u : 0u; F.vcf_columns = O.vcf_columns ? 1u : 0u;
    hipLaunchKernelGGL(sv_plen, dim3(blocks_of(m)), dim3(256), 0, st, F);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    if (O.want_text) {
      if (lra_exclusive_scan<uint32_t>(ctx, (long)(4 * nk), plen.p, poff.p)) return fail(LRA_ERR_HIP, "lra_bam_svcalls: a scan failed");
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(&total, poff.p + 4 * nk, 8, hipMemcpyDeviceToHost, st));
      LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    if (!lra_sv_piece_bytes(nk, total, (int)O.want_text, (int)O.want_values, &dev_text, &host_text, &value_bytes))
      return fail(LRA_ERR_NOMEM, "lra_bam_svcalls: a piece of %llu rows and %llu bytes of text is beyond this machine's addresses", (unsigned long long)nk, (unsigned long long)total);
    if (O.want_text && !grab(text, dev_text)) return fail(LRA_ERR_NOMEM, "lra_bam_svcalls: hipMalloc of %llu bytes for a piece's text failed", (unsigned long long)total);
    if (O.want_values && !grab(vals, nk)) return fail(LRA_ERR_NOMEM, "lra_bam_svcalls: hipMalloc failed for %llu rows", (unsigned long long)nk);
    F.text = O.want_text ? text.p : nullptr; F.n_text = total; F.vals = O.want_values ? vals.p : nullptr;
    if (nk) {
      hipLaunchKernelGGL(sv_small, dim3(blocks_of(nk)), dim3(256), 0, st, F);
      if (O.want_text) hipLaunchKernelGGL(sv_bulk, dim3(wave_blocks(ctx, (total + SV_CHUNK - 1) / SV_CHUNK)), dim3(256), 0, st, F);
    }
    LRA_HIP_CHECK(ctx, hipGetLastError());
    S.ms_emit += T.stop();
  }
  {
    Timer T(st);
    if (O.want_text) {
      if (!h_text.ensure(host_text, 0, st)) return fail(LRA_ERR_NOMEM, "lra_bam_svcalls: hipHostMalloc of %llu bytes for a piece's text failed", (unsigned long long)total);
      if (total) LRA_HIP_CHECK(ctx, hipMemcpyAsync(h_text.p, text.p, total, hipMemcpyDeviceToHost, st));
    }
    if (O.want_values && nk) {
      if (!h_vals.ensure(nk, 0, st)) return fail(LRA_ERR_NOMEM, "lra_bam_svcalls: hipHostMalloc failed for %llu rows", (unsigned long long)nk);
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(h_vals.p, vals.p, value_bytes, hipMemcpyDeviceToHost, st));
    }
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    S.ms_copy += T.stop();
  }
  S.bytes_text += total;
  piece->n_rows = nk; piece->rows = O.want_values && nk ? h_vals.p : nullptr; piece->text = total ? h_text.p : nullptr; piece->text_len = total; piece->kind = (uint32_t)k;
  return LRA_OK;
}

// The kept rows of finish_kind's F go behind the sink's table of kind k, device to device, with their bytes; the piece says only how many.
int lra_bam_svcalls::to_sink(int k, SvF& F, uint64_t nk, struct lra_bam_svcalls_piece* piece) {
  hipStream_t st = ctx->stream;
  lra_sv_sink& K = *sink;
  Timer T(st);
  F.nk = nk; F.plen = nullptr; F.bytes = bytes[k][cur[k]].p;
  hipLaunchKernelGGL(sv_plen, dim3(blocks_of(F.m)), dim3(256), 0, st, F);   // (kidx: the kept rows in NR order)
  LRA_HIP_CHECK(ctx, hipGetLastError());
  if (nk) {
    uint64_t nb = 0;
    if (!grab(s_len, nk) || !grab(s_off, nk + 1)) return fail(LRA_ERR_NOMEM, "lra_bam_svcalls: hipMalloc failed for %llu rows", (unsigned long long)nk);
    hipLaunchKernelGGL(sv_sink_len, dim3(blocks_of(nk)), dim3(256), 0, st, F, s_len.p);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    if (lra_exclusive_scan<uint32_t>(ctx, (long)nk, s_len.p, s_off.p)) return fail(LRA_ERR_HIP, "lra_bam_svcalls: a scan failed");
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&nb, s_off.p + nk, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (!K.rows[k].ensure(K.n_rows[k] + nk, K.n_rows[k], st) || !K.bytes[k].ensure(K.n_bytes[k] + nb + 8, K.n_bytes[k], st))
      return fail(LRA_ERR_NOMEM, "lra_bam_svcalls: hipMalloc failed for %llu kept rows and %llu bytes of names and ALT", (unsigned long long)(K.n_rows[k] + nk), (unsigned long long)(K.n_bytes[k] + nb));
    hipLaunchKernelGGL(sv_sink_copy, dim3(wave_blocks(ctx, nk)), dim3(256), 0, st, F, (const uint64_t*)s_off.p, K.rows[k].p, K.n_rows[k], K.bytes[k].p, K.n_bytes[k]);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    K.n_rows[k] += nk; K.n_bytes[k] += nb;
  }
  S.ms_copy += T.stop();
  piece->n_rows = nk; piece->kind = (uint32_t)k;
  return LRA_OK;
}

// the rows [0, m) of kind k leave the table
int lra_bam_svcalls::pop(int k, uint64_t m) {
  hipStream_t st = ctx->stream;
  if (!m) return LRA_OK;
  const uint64_t left = n_rows[k] - m;
  if (!left) { n_rows[k] = 0; n_bytes[k] = 0; return LRA_OK; }
  const int to = cur[k] ^ 1;
  if (!rows[k][to].ensure(left, 0, st)) return fail(LRA_ERR_NOMEM, "lra_bam_svcalls: hipMalloc failed for %llu rows", (unsigned long long)left);
  unsigned long long base = 0;
  hipLaunchKernelGGL(sv_pop, dim3(blocks_of(left)), dim3(256), 0, st, (const SvRow*)rows[k][cur[k]].p, rows[k][to].p, m, n_rows[k], sv_misc.p + M_BASE);
  LRA_HIP_CHECK(ctx, hipGetLastError());
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&base, sv_misc.p + M_BASE, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  const uint64_t nb = n_bytes[k] - base;
  if (!bytes[k][to].ensure(nb + 8, 0, st)) return fail(LRA_ERR_NOMEM, "lra_bam_svcalls: hipMalloc of %llu bytes for the rows' names and ALT failed", (unsigned long long)nb);
  if (nb) LRA_HIP_CHECK(ctx, hipMemcpyAsync(bytes[k][to].p, bytes[k][cur[k]].p + base, nb, hipMemcpyDeviceToDevice, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  cur[k] = to; n_rows[k] = left; n_bytes[k] = nb;
  return LRA_OK;
}

int lra_bam_svcalls::next(struct lra_bam_svcalls_piece* piece) {
  hipStream_t st = ctx->stream;
  memset(piece, 0, sizeof *piece);
  if (!over) if (int rc = take_genome("lra_bam_svcalls_next")) { over = true; faulted = true; return rc; }   // (the context may have taken another genome since)
  if (sink) { sink->rname = (const char*)rname.p; sink->rname_off = rname_off.p; sink->genome = d_genome; }
  for (;;) {
    if (fin_stage == 0 && !faulted && (n_rows[0] || n_rows[1])) {
      // the lowest reference in the tables; it is final when a record of a later one has been delivered, or the pass is over
      int32_t r[2] = {INT32_MAX, INT32_MAX};
      for (int k = 0; k < 2; k++)
        if (n_rows[k]) LRA_HIP_CHECK(ctx, hipMemcpyAsync(&r[k], (const char*)rows[k][cur[k]].p + offsetof(SvRow, ref), 4, hipMemcpyDeviceToHost, st));
      LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
      const int32_t lowest = std::min(r[0], r[1]);
      const bool seen_later = has_last && (uint32_t)(last_key >> 32) > (uint32_t)lowest;   // (refID -1, the unmapped tail, is later than every reference)
      if (over || seen_later) {
        unsigned long long m[2] = {0, 0};
        for (int k = 0; k < 2; k++) {
          if (!n_rows[k]) continue;
          LRA_HIP_CHECK(ctx, hipMemsetAsync(sv_misc.p + M_PREFIX, 0, 8, st));
          hipLaunchKernelGGL(sv_prefix, dim3(blocks_of(n_rows[k])), dim3(256), 0, st, (const SvRow*)rows[k][cur[k]].p, n_rows[k], lowest, sv_misc.p + M_PREFIX);
          LRA_HIP_CHECK(ctx, hipGetLastError());
          LRA_HIP_CHECK(ctx, hipMemcpyAsync(&m[k], sv_misc.p + M_PREFIX, 8, hipMemcpyDeviceToHost, st));
          LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
        }
        fin_ref = lowest; fin_m[0] = m[0]; fin_m[1] = m[1]; fin_stage = 1;
      }
    }
    if (fin_stage == 1 || fin_stage == 2) {                     // the DEL piece, then the INS piece
      const int k = fin_stage == 1 ? 1 : 0;
      fin_stage++;
      if (fin_m[k]) {
        if (int rc = finish_kind(k, fin_m[k], piece)) { faulted = true; return rc; }
        piece->ref_id = fin_ref;
        if (piece->n_rows) return LRA_OK;                      // (n_rows == 0 cannot be: the lowest NR of a reference is always kept; the test costs nothing)
      }
      continue;
    }
    if (fin_stage == 3) {
      fin_stage = 0;
      for (int k = 0; k < 2; k++) if (int rc = pop(k, fin_m[k])) { faulted = true; return rc; }
      continue;
    }
    if (over) { n_rows[0] = n_rows[1] = 0; return LRA_OK; }     // the pass is over: the end piece (what a fault left unfinished is dropped)
    int state = 0;
    if (int rc = step(*this, &state)) { faulted = true; return rc; }
  }
}

static_assert(sizeof(struct lra_bam_svcalls_row) == LRA_SV_VALUE_BYTES, "lra_bam_svcalls_row");

extern "C" int lra_bam_svcalls_create(lra_ctx* ctx, const char* bam_path, const char* bai_path, const struct lra_bam_svcalls_opts* opts, lra_bam_svcalls** out) {
  if (!ctx || !bam_path || !out) return LRA_ERR_INVALID;
  *out = nullptr;
  std::unique_ptr<lra_bam_svcalls> d(new lra_bam_svcalls());
  if (opts) d->O = *opts; else { d->O.exclude = ~0u; d->O.want_text = 1; d->O.drop_contained = 1; d->O.min_size = 40; }
  d->rules = lra_vcf_rules_of(d->O.require, d->O.exclude, d->O.min_mapq, lra_sv_min_size(d->O.min_size), 0);
  if (!d->O.want_text && !d->O.want_values) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_bam_svcalls_create: neither text nor values are wanted");
  if (!lra_sv_name_ok(d->O.aligner) || !lra_sv_name_ok(d->O.hap)) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_bam_svcalls_create: aligner and hap are printable words without blanks");
  for (int k = 0; k < 2; k++) d->stem[k] = lra_sv_id_stem(d->O.aligner, d->O.hap, k);
  d->O.aligner = d->O.hap = nullptr;                           // (the caller's strings are not kept)
  int rc = d->open_files(ctx, "lra_bam_svcalls", bam_path, bai_path, d->O.window_bytes);
  if (!rc) rc = d->take_genome("lra_bam_svcalls_create");
  if (!rc) rc = d->set_mask(0, nullptr, nullptr, nullptr);
  bool ok = !rc && d->zero_misc() && d->sv_misc.ensure(M_WORDS);
  for (int k = 0; ok && k < 2; k++)
    ok = d->d_stem[k].ensure(d->stem[k].size() + 1) && hipMemcpyAsync(d->d_stem[k].p, d->stem[k].data(), d->stem[k].size(), hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
  ok = ok && hipStreamSynchronize(ctx->stream) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    return pass_create_failed(d.get(), rc ? rc : lra_set_err(ctx, LRA_ERR_NOMEM, "lra_bam_svcalls_create: hipMalloc failed"));
  }
  *out = d.release();
  return LRA_OK;
}

__attribute__((visibility("hidden"))) void lra_bam_svcalls_set_sink(lra_bam_svcalls* d, lra_sv_sink* sink) { d->sink = sink; }

extern "C" void lra_bam_svcalls_destroy(lra_bam_svcalls* d) { pass_destroy(d); }

extern "C" int lra_bam_svcalls_header(lra_bam_svcalls* d, int* n_ref, const char* const** names, const uint64_t** ref_len) {
  return d ? d->header_refs(n_ref, names, ref_len) : LRA_ERR_INVALID;
}

extern "C" int lra_bam_svcalls_set_mask(lra_bam_svcalls* d, uint64_t n, const int32_t* ref_id, const int64_t* beg, const int64_t* end) {
  if (!d || (n && (!ref_id || !beg || !end))) return LRA_ERR_INVALID;
  LRA_HIP_CHECK(d->ctx, hipSetDevice(d->ctx->device));
  d->over = true;                                              // (a pass in hand ends: its rows were tested against the mask before)
  return d->set_mask(n, ref_id, beg, end);
}

extern "C" int lra_bam_svcalls_all(lra_bam_svcalls* d) {
  if (!d) return LRA_ERR_INVALID;
  d->over = true;
  if (int rc = d->take_genome("lra_bam_svcalls_all")) return rc;
  if (int rc = d->pass_all()) return rc;
  return d->begin_pass();
}

extern "C" int lra_bam_svcalls_region(lra_bam_svcalls* d, int32_t ref_id, int64_t beg, int64_t end) {
  if (!d) return LRA_ERR_INVALID;
  d->over = true;
  if (int rc = d->take_genome("lra_bam_svcalls_region")) return rc;
  if (ref_id >= 0 && ref_id < d->refs.n_ref && !lra_sv_whole_reference(beg, end, d->refs.len[(size_t)ref_id]))
    return lra_set_err(d->ctx, LRA_ERR_INVALID, "lra_bam_svcalls_region: [%lld, %lld) is not the whole of reference %d (%llu bases): the merge and the numbering need every row of it",
                       (long long)beg, (long long)end, (int)ref_id, (unsigned long long)d->refs.len[(size_t)ref_id]);
  if (int rc = d->pass_region(ref_id, beg, end)) return rc;
  return d->begin_pass();
}

extern "C" int lra_bam_svcalls_next(lra_bam_svcalls* d, struct lra_bam_svcalls_piece* piece) {
  if (!d || !piece) return LRA_ERR_INVALID;
  LRA_HIP_CHECK(d->ctx, hipSetDevice(d->ctx->device));
  return d->next(piece);
}

extern "C" int lra_bam_svcalls_stats(lra_bam_svcalls* d, struct lra_bam_svcalls_stats* out) {
  if (!d || !out) return LRA_ERR_INVALID;
  *out = d->S;
  d->add_stats(out);
  return LRA_OK;
}

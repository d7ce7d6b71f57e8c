// lra_amd/csrc/bam_vcf_walk.h -- the variant walk over a window's framed records that lra_bam_vcf (bam_vcf.hip: every insertion and deletion as a VCF line)
// and lra_bam_svcalls (bam_svcalls.hip: the assembly SV tables) share: the kernels from the record checks to the compacted variants, and lra_vcf_walk,
// the arrays they run on and the stages in order.  include/lra_hip.h has the rules under lra_bam_vcf; bam_vcf_host.h the arithmetic host and kernels share;
// bam_contained.h the filter in front of the walk.  The kernels are TU-local, as scan.h's and bam_rec.h's are.
//
// records.  The pass's front (bam_pass.h: Front, rec_check, rec_in_region, rec_cut; its refuse): rec_check, a lane per framed record: the record's
// arithmetic; bs_span gives a region pass every record's span for the overlap test.  vc_select, a lane per record: the contained filter's flag, the filters
// (rec_in_region: the overlap and the first record at or behind the region's end; rec_cut behind it), and where the ops are (ops_of, bam_rec.h: depth's
// rule).  One scan of the op counts.
// the walk.  A lane per op, never a lane or a wave per record: one record of millions of ops is as many lanes as a thousand records of three.
// vc_opinfo: the op's advance in SEQ (M I S = X) and on the reference (M D N = X) and its class -- match, ins (I S), del (D N), none (H P, length 0).
// Two scans over all ops of the window give (q, r) in front of every op; less their values at the record's first op they are the record's counters: the
// segmented scan.  The ops of a class are numbered by one scan and vc_live writes their classes side by side, so the op of a class in front of an op is
// one read however many ops of class none stand between; vc_heads marks the op that begins a maximal run of one class (ops of class none do not part a
// run: I P I is one); one scan numbers the runs, vc_groups writes them.  One scan of "is a match run" numbers the match runs, vc_anchor stores where in SEQ each ends: the run in front of
// insertion or deletion run g is match run mcnt[g] - 1 however many ins / del runs alternate in between, and none when that count is the record's first.
// vc_rec, a lane per record: walked or skipped, the sums against l_seq and the reference's length.
// variants.  variant_of, per run: an ins / del run of a walked record with a match run in front and another run behind; its lengths, the region test of
// the anchor, min_length (count_small: the runs that fail it alone are counted by kind).  vc_vkeep flags, one scan compacts, vc_compact writes the variant
// and, for a consumer that prints lra_bam_vcf's line, the lengths of its four pieces.
#pragma once
#include "common.h"
#include "scan.h"
#include "bam_pass.h"
#include "bam_keys.h"
#include "bam_contained.h"
#include "bam_vcf_host.h"
#include "seed_state.h"
#include "map_state.h"

namespace {

enum { C_NONE = 0, C_MATCH = 1, C_INS = 2, C_DEL = 3 };
enum { S_FILTERED = 0, S_SKIPPED = 1, S_CAND = 2 };
enum { B_KINDS = B_OWN };                                      // bad[] behind the pass's words: bam_vcf_host.h's kinds
static_assert(S_FILTERED == 0, "rec_cut clears state[] to S_FILTERED");
enum { N_WALKED = 0, N_SKIPPED = 1, N_INS = 2, N_DEL = 3, N_CONTAINED = 4, N_SMALL_INS = 5, N_SMALL_DEL = 6, N_CNT = 7 };    // cnt[]

struct Var {                                                  // a kept variant
  uint64_t rec, seq_at, name_at, aq, g_at, ref_len, alt_len;  // its record; where SEQ and the name are in the window's data; the anchor's SEQ index; REF's first byte in the genome
  int64_t svlen; int32_t ref, anchor; uint32_t del, l_name, flag, pad;
};

struct Vc {                                                   // what the kernels of a window see
  Front F;                                                    // (bam_pass.h) record i is F.data[F.pos[i], F.pos[i + 1])
  lra_vcf_rules rules; int count_small;
  const char* rname; const uint64_t* rname_off;
  const unsigned char* genome; const uint64_t* chrom_pos;
  uint32_t* state; const uint32_t* drop;               // drop: bam_contained.h's flags, or null
  uint32_t* c_op; uint64_t* op_off; uint64_t* ops_src; uint32_t* has_m; uint32_t* walked;
  uint32_t* qadv; uint32_t* radv; uint8_t* cls; uint8_t* lcls; uint32_t* orec; uint32_t* head; uint64_t* Q; uint64_t* R; uint64_t* hoff; uint64_t n_op;
  uint64_t* g_op; uint32_t* g_m; uint64_t* mcnt; uint64_t* m_end; uint32_t* vkeep; uint64_t* voff; uint64_t n_grp;
  Var* var; uint32_t* plen; uint64_t* poff; uint64_t n_var;
  struct lra_bam_vcf_variant* vals; uint64_t ord_base;
  unsigned char* text; uint64_t n_text;
  unsigned long long* cnt;
};

__device__ __forceinline__ uint32_t class_of(uint32_t code, uint32_t len) {
  if (!len) return C_NONE;
  return code == 0 || code == 7 || code == 8 ? C_MATCH : code == 1 || code == 4 ? C_INS : code == 2 || code == 3 ? C_DEL : C_NONE;
}

__global__ void __launch_bounds__(256) vc_select(Vc V) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V.F.n) return;
  const uint64_t at0 = V.F.pos[i];
  const Core c = core_of(V.F.data + at0);
  bool pass = c.ref >= 0 && !(V.drop && V.drop[i]) && (c.flag & V.rules.require) == V.rules.require && (c.flag & V.rules.exclude) == 0 && c.mapq >= V.rules.min_mapq;
  if (V.F.region) pass = rec_in_region(V.F, i, c.ref, c.pos) && pass;
  bool cand = pass && c.n_cig >= 1 && c.l_seq > 0;
  uint64_t ops = at0 + 36 + c.l_name; uint32_t n_op = c.n_cig;
  if (cand && !ops_of(V.F.data, at0, V.F.pos[i + 1], c, &ops, &n_op)) { atomicMin(&V.F.bad[B_KINDS + LRA_VCF_BAD_AUX], (unsigned long long)i); cand = false; }
  cand = cand && n_op >= 1;
  V.state[i] = !pass ? S_FILTERED : cand ? S_CAND : S_SKIPPED;
  V.c_op[i] = cand ? n_op : 0u; V.ops_src[i] = ops; V.has_m[i] = 0u;
}

__global__ void __launch_bounds__(256) vc_opinfo(Vc V) {
  const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= V.n_op) return;
  const uint64_t r = last_le(V.op_off, V.F.n, o);
  const uint32_t op = le32(V.F.data + V.ops_src[r] + 4 * (o - V.op_off[r]));
  const uint32_t code = op & 15u, len = op >> 4;
  if (code > 8u) atomicMin(&V.F.bad[B_KINDS + LRA_VCF_BAD_OP], (unsigned long long)r);
  const uint32_t c = code > 8u ? (uint32_t)C_NONE : class_of(code, len);
  V.cls[o] = (uint8_t)c; V.orec[o] = (uint32_t)r; V.head[o] = c != C_NONE ? 1u : 0u;   // (head: until vc_heads, "has a class")
  V.qadv[o] = c == C_MATCH || c == C_INS ? len : 0u;
  V.radv[o] = c == C_MATCH || c == C_DEL ? len : 0u;
  if (c == C_MATCH) V.has_m[r] = 1u;                           // (every writer writes 1)
}

// hoff numbers the ops of a class (the scan of head as vc_opinfo left it): their classes side by side
__global__ void __launch_bounds__(256) vc_live(Vc V) {
  const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o < V.n_op && V.cls[o] != C_NONE) V.lcls[V.hoff[o]] = V.cls[o];
}

// the op begins a run: the op of a class in front of it in the record, the ops of class none skipped, has another class or is not there
__global__ void __launch_bounds__(256) vc_heads(Vc V) {
  const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= V.n_op) return;
  const uint32_t c = V.cls[o];
  uint32_t h = 0;
  if (c != C_NONE) {
    const uint64_t k = V.hoff[o], k0 = V.hoff[V.op_off[V.orec[o]]];   // its number among the ops of a class, and the record's first
    h = k == k0 || V.lcls[k - 1] != c ? 1u : 0u;
  }
  V.head[o] = h;
}

// a lane per record: a candidate with an M = X base is walked; its ops against l_seq and its reference
__global__ void __launch_bounds__(256) vc_rec(Vc V) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool walked = false, skipped = false, contained = false;
  if (i < V.F.n) {
    const uint32_t st = V.state[i];
    if (V.drop && V.drop[i]) contained = !V.F.region || (i < V.F.bad[B_STOP] && (int32_t)le32(V.F.data + V.F.pos[i] + 4) == V.F.ref_id);
    walked = st == S_CAND && V.has_m[i];
    skipped = st == S_SKIPPED || (st == S_CAND && !walked);
    V.walked[i] = walked ? 1u : 0u;
    if (walked) {
      const Core c = core_of(V.F.data + V.F.pos[i]);
      const uint64_t o0 = V.op_off[i], o1 = V.op_off[i + 1];
      if (V.Q[o1] - V.Q[o0] != (uint64_t)c.l_seq) atomicMin(&V.F.bad[B_KINDS + LRA_VCF_BAD_SEQ], (unsigned long long)i);
      const uint64_t len = V.chrom_pos[c.ref + 1] - V.chrom_pos[c.ref];
      if (c.pos < 0 || (uint64_t)c.pos + (V.R[o1] - V.R[o0]) > len) atomicMin(&V.F.bad[B_KINDS + LRA_VCF_BAD_SPAN], (unsigned long long)i);
    }
  }
  const unsigned long long bw = __ballot(walked), bs = __ballot(skipped), bc = __ballot(contained);
  if ((threadIdx.x & 63) == 0) {
    if (bc) atomicAdd(&V.cnt[N_CONTAINED], (unsigned long long)__popcll(bc));
    if (bw) atomicAdd(&V.cnt[N_WALKED], (unsigned long long)__popcll(bw));
    if (bs) atomicAdd(&V.cnt[N_SKIPPED], (unsigned long long)__popcll(bs));
  }
}

__global__ void __launch_bounds__(256) vc_groups(Vc V) {
  const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= V.n_op || !V.head[o]) return;
  const uint64_t g = V.hoff[o];
  V.g_op[g] = o; V.g_m[g] = V.cls[o] == C_MATCH ? 1u : 0u;
}

// where in the window's q a match run ends: in front of the run behind it, or at the record's end
__global__ void __launch_bounds__(256) vc_anchor(Vc V) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= V.n_grp || !V.g_m[g]) return;
  const uint32_t r = V.orec[V.g_op[g]];
  const bool more = g + 1 < V.n_grp && V.orec[V.g_op[g + 1]] == r;
  V.m_end[V.mcnt[g]] = V.Q[more ? V.g_op[g + 1] : V.op_off[r + 1]];
}

// *small (optional): 1 / 2 for an insertion / deletion that is a variant in everything but min_length
__device__ __forceinline__ bool variant_of(const Vc& V, uint64_t g, Var* out, int* small = nullptr) {
  const uint64_t o = V.g_op[g];
  const uint32_t c = V.cls[o];
  if (c != C_INS && c != C_DEL) return false;
  const uint32_t r = V.orec[o];
  if (!V.walked[r] || g + 1 >= V.n_grp) return false;
  const uint64_t o2 = V.g_op[g + 1];
  if (V.orec[o2] != r) return false;                           // the run reaches the end of the CIGAR
  const uint64_t o0 = V.op_off[r];
  if (V.mcnt[g] == V.mcnt[V.hoff[o0]]) return false;           // no M = X base in front of it
  const uint64_t at0 = V.F.pos[r];
  const Core k = core_of(V.F.data + at0);
  const uint64_t qb = V.Q[o0], rb = V.R[o0];
  const uint64_t aq = V.m_end[V.mcnt[g] - 1] - 1 - qb, q1 = V.Q[o2] - qb;
  const int64_t r0 = (int64_t)k.pos + (int64_t)(V.R[o] - rb), r1 = (int64_t)k.pos + (int64_t)(V.R[o2] - rb);
  const lra_vcf_shape s = lra_vcf_shape_of(c == C_DEL, aq, r0, q1, r1);
  if (!lra_vcf_anchor_in(V.F.region, r0 - 1, V.F.beg, V.F.end)) return false;
  if (!lra_vcf_long_enough(s.svlen, V.rules.min_length)) { if (small) *small = c == C_DEL ? 2 : 1; return false; }
  if (out) {
    out->rec = r; out->name_at = at0 + 36; out->seq_at = at0 + 36 + k.l_name + 4ull * k.n_cig; out->aq = aq;
    out->g_at = V.chrom_pos[k.ref] + (uint64_t)(r0 - 1); out->ref_len = s.ref_len; out->alt_len = s.alt_len; out->svlen = s.svlen;
    out->ref = k.ref; out->anchor = (int32_t)(r0 - 1); out->del = c == C_DEL; out->l_name = k.l_name - 1; out->flag = k.flag; out->pad = 0;
  }
  return true;
}

__global__ void __launch_bounds__(256) vc_vkeep(Vc V) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int small = 0;
  if (g < V.n_grp) V.vkeep[g] = variant_of(V, g, nullptr, &small) ? 1u : 0u;
  if (!V.count_small) return;                                  // (uniform)
  // the block's counts in LDS first: nearly every wave of a read set has some, and one pair of atomics a block is a quarter of one a wave
  __shared__ unsigned int n_small[2];
  if (threadIdx.x < 2) n_small[threadIdx.x] = 0;
  __syncthreads();
  const unsigned long long bi = __ballot(small == 1), bd = __ballot(small == 2);
  if ((threadIdx.x & 63) == 0) {
    if (bi) atomicAdd(&n_small[0], (unsigned int)__popcll(bi));
    if (bd) atomicAdd(&n_small[1], (unsigned int)__popcll(bd));
  }
  __syncthreads();
  if (threadIdx.x < 2 && n_small[threadIdx.x]) atomicAdd(&V.cnt[N_SMALL_INS + threadIdx.x], (unsigned long long)n_small[threadIdx.x]);
}

#define LIT_LEN(s) ((uint32_t)sizeof(s) - 1u)
#define T_QUAL "\t60\t"
#define T_PASS "PASS\t"
#define T_SVTYPE "SVTYPE="
#define T_SVLEN ";SVLEN="
#define T_QNAME ";QNAME="
#define T_QSTART ";QSTART="
#define T_QSTRAND ";QSTRAND="
#define T_END "\tGT\t1/1\n"
template <size_t N> __device__ __forceinline__ unsigned char* put_lit(unsigned char* d, const char (&s)[N]) {
  for (size_t k = 0; k + 1 < N; k++) d[k] = (unsigned char)s[k];
  return d + (N - 1);
}
// the INFO column, SVTYPE= through QSTRAND's sign
__device__ __forceinline__ uint32_t info_body_len(int64_t svlen, uint32_t l_name, uint64_t qstart) {
  return LIT_LEN(T_SVTYPE) + 3u + LIT_LEN(T_SVLEN) + (uint32_t)slen(svlen) + LIT_LEN(T_QNAME) + l_name + LIT_LEN(T_QSTART) + (uint32_t)ndig(qstart) + LIT_LEN(T_QSTRAND) + 1u;
}
__device__ __forceinline__ unsigned char* put_info_body(unsigned char* d, bool del, int64_t svlen, const uint8_t* name, uint32_t l_name, uint64_t qstart, bool reverse) {
  d = put_lit(d, T_SVTYPE);
  if (del) d = put_lit(d, "DEL"); else d = put_lit(d, "INS");
  d = put_lit(d, T_SVLEN); d = put_s(d, svlen);
  d = put_lit(d, T_QNAME);
  for (uint32_t k = 0; k < l_name; k++) *d++ = name[k];
  d = put_lit(d, T_QSTART); d = put_u(d, qstart);
  d = put_lit(d, T_QSTRAND); *d++ = reverse ? '-' : '+';
  return d;
}
// the bytes of a line from "\t60\tPASS\t" through the newline, which both consumers print alike
__device__ __forceinline__ uint32_t info_len(int64_t svlen, uint32_t l_name, uint64_t qstart) {
  return LIT_LEN(T_QUAL) + LIT_LEN(T_PASS) + info_body_len(svlen, l_name, qstart) + LIT_LEN(T_END);
}
__device__ __forceinline__ void put_info(unsigned char* d, bool del, int64_t svlen, const uint8_t* name, uint32_t l_name, uint64_t qstart, bool reverse) {
  d = put_lit(d, T_QUAL); d = put_lit(d, T_PASS);
  d = put_info_body(d, del, svlen, name, l_name, qstart, reverse);
  put_lit(d, T_END);
}

__global__ void __launch_bounds__(256) vc_compact(Vc V) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= V.n_grp || !V.vkeep[g]) return;
  Var v;
  variant_of(V, g, &v);
  const uint64_t j = V.voff[g];
  V.var[j] = v;
  if (!V.plen) return;
  const uint32_t name = (uint32_t)(V.rname_off[v.ref + 1] - V.rname_off[v.ref]);
  V.plen[4 * j] = name + 1u + (uint32_t)ndig((uint64_t)v.anchor + V.rules.pos_one_based) + 3u;
  // (32 bits hold every piece: a record's bytes are below 2^32, so l_seq + (l_seq + 1) / 2 is, and 1 + alt_len <= 1 + l_seq < 2^32; ref_len <= the
  // reference's length, below 2^31.  The scan's total is 64 bits.)
  V.plen[4 * j + 1] = (uint32_t)v.ref_len;
  V.plen[4 * j + 2] = 1u + (uint32_t)v.alt_len;
  V.plen[4 * j + 3] = info_len(v.svlen, v.l_name, v.aq + 1);
}

// the context's genome against the file's reference table; the kernels' pointers to it
inline int lra_vcf_take_genome(lra_bam_pass& P, const char* fn, const unsigned char** genome, const uint64_t** chrom_pos) {
  lra_ctx* ctx = P.ctx;
  lra_seed_state* s = ctx->seed; lra_map_state* m = ctx->map;
  if (!s || !s->genome || !m || m->chrom_pos.size() < 2 || !m->d_chrom_pos)
    return lra_set_err(ctx, LRA_ERR_INVALID, "%s: the context has no genome and chromosome table loaded (lra_ctx_load_genome, lra_ctx_load_chromosomes)", fn);
  std::string why;
  const int64_t at = lra_vcf_table_diff(m->chrom_pos, s->genome_len, P.refs.len, &why);
  if (at >= 0) {
    const std::string name = at < P.refs.n_ref ? " (" + P.refs.name[(size_t)at] + ")" : std::string();
    return lra_set_err(ctx, LRA_ERR_INVALID, "%s: %s: reference %lld%s: %s", fn, P.path.c_str(), (long long)at, name.c_str(), why.c_str());
  }
  *genome = s->genome; *chrom_pos = m->d_chrom_pos;
  return LRA_OK;
}

// The walk's arrays and its stages for a consumer `P` of the pass.  The times go where the consumer's stats point.
struct lra_vcf_walk {
  Buf<uint32_t> state, c_op, has_m, walked, qadv, radv, orec, head, g_m, vkeep, plen; Buf<uint8_t> cls, lcls;
  Buf<uint64_t> op_off, ops_src, Q, R, hoff, g_op, mcnt, m_end, voff, poff; Buf<Var> var;
  lra_contained CT; bool ct_fault = false;
  double* ms_frame_select = nullptr; double* ms_ops = nullptr; double* ms_walk = nullptr; double* ms_lengths = nullptr;

  void release() {
    state.release(); c_op.release(); has_m.release(); walked.release(); qadv.release(); radv.release(); orec.release(); head.release();
    g_m.release(); vkeep.release(); plen.release(); cls.release(); lcls.release(); op_off.release(); ops_src.release(); Q.release();
    R.release(); hoff.release(); g_op.release(); mcnt.release(); m_end.release(); voff.release(); poff.release(); var.release(); CT.release();
  }
  // a pass begins
  int begin(lra_bam_pass& P, bool drop_contained) {
    ct_fault = false;
    if (drop_contained && !CT.begin(P.ctx->stream)) return P.fail(LRA_ERR_HIP, "%s: the contained filter could not be set up", P.who);
    return LRA_OK;
  }
  void forget() { CT.forget(); }
  // the window is delivered
  void commit(lra_bam_pass& P) { if (!CT.commit(P.ctx->stream)) ct_fault = true; }   // (the next window refuses)

  // The records' arithmetic (the pass's front_check).  V: the caller has zeroed it and set what is its own (rules, count_small, genome, chrom_pos, ord_base); the
  // pass's fields and the arrays are set here.  *bad_idx < n: the lowest record that is refused.
  int check(lra_bam_pass& P, Vc& V, uint64_t n, uint64_t limit, uint64_t* bad_idx, uint64_t* bad_pos, std::string* bad_why) {
    lra_ctx* ctx = P.ctx; hipStream_t st = ctx->stream;
    *bad_idx = NONE;
    if (ct_fault) return P.fail(LRA_ERR_HIP, "%s: the contained filter's carry could not be kept", P.who);
    V.rname = (const char*)P.rname.p; V.rname_off = P.rname_off.p;
    if (!(P.grab(state, n) && P.grab(c_op, n) && P.grab(op_off, n + 1) && P.grab(ops_src, n) && P.grab(has_m, n) && P.grab(walked, n)))
      return P.fail(LRA_ERR_NOMEM, "%s: hipMalloc failed for the arrays of %llu records", P.who, (unsigned long long)n);
    V.state = state.p; V.c_op = c_op.p; V.op_off = op_off.p; V.ops_src = ops_src.p; V.has_m = has_m.p; V.walked = walked.p;
    V.cnt = (unsigned long long*)(P.misc.p + MISC_CNT);
    Timer T(st);
    LRA_HIP_CHECK(ctx, hipMemsetAsync(V.cnt, 0, 8 * N_CNT, st));
    const int rc = P.front_check(V.F, n, limit, bad_idx, bad_pos, bad_why);
    *ms_frame_select += T.stop();
    return rc;
  }

  // Behind check(): the filter, the select, the ops, the runs, the variants.  *nv variants stand in var.p; with want_plen their lines' pieces are placed (poff.p) and
  // *total is the text's bytes.  cnt[N_CNT]: the window's counts so far (N_INS and N_DEL are the emitter's).
  int walk(lra_bam_pass& P, Vc& V, bool drop_contained, bool want_plen, uint64_t* bad_idx, uint64_t* bad_pos, std::string* bad_why, uint64_t* stop_idx, uint64_t* nv, uint64_t* total,
           uint64_t* cnt) {
    lra_ctx* ctx = P.ctx; hipStream_t st = ctx->stream;
    const uint64_t n = V.F.n;
    *stop_idx = NONE; *nv = 0; *total = 0;
    unsigned long long res[B_WORDS];
    uint64_t n_op = 0;
    {
      Timer T(st);
      if (drop_contained) {
        if (!CT.window(st, V.F.data, V.F.pos, n, V.F.region ? V.F.limit : ~0ull)) return P.fail(LRA_ERR_NOMEM, "%s: the contained filter of %llu records failed", P.who, (unsigned long long)n);
        V.drop = CT.drop.p;
      }
      P.front_span(V.F);
      hipLaunchKernelGGL(vc_select, dim3(blocks_of(n)), dim3(256), 0, st, V);
      P.front_cut(V.F, V.state, V.c_op);
      LRA_HIP_CHECK(ctx, hipGetLastError());
      if (lra_exclusive_scan<uint32_t>(ctx, (long)n, c_op.p, op_off.p)) return P.fail(LRA_ERR_HIP, "%s: a scan failed", P.who);
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(&n_op, op_off.p + n, 8, hipMemcpyDeviceToHost, st));
      LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
      *ms_frame_select += T.stop();
    }
    uint64_t n_grp = 0;
    {
      Timer T(st);
      if (!(P.grab(qadv, n_op + 1) && P.grab(radv, n_op + 1) && P.grab(cls, n_op + 1) && P.grab(lcls, n_op + 1) && P.grab(orec, n_op + 1) && P.grab(head, n_op + 1) && P.grab(Q, n_op + 1) &&
            P.grab(R, n_op + 1) && P.grab(hoff, n_op + 1)))
        return P.fail(LRA_ERR_NOMEM, "%s: hipMalloc failed for %llu CIGAR ops", P.who, (unsigned long long)n_op);
      V.qadv = qadv.p; V.radv = radv.p; V.cls = cls.p; V.lcls = lcls.p; V.orec = orec.p; V.head = head.p; V.Q = Q.p; V.R = R.p; V.hoff = hoff.p; V.n_op = n_op;
      if (n_op) hipLaunchKernelGGL(vc_opinfo, dim3(blocks_of(n_op)), dim3(256), 0, st, V);
      LRA_HIP_CHECK(ctx, hipGetLastError());
      if (lra_exclusive_scan<uint32_t>(ctx, (long)n_op, qadv.p, Q.p) || lra_exclusive_scan<uint32_t>(ctx, (long)n_op, radv.p, R.p)) return P.fail(LRA_ERR_HIP, "%s: a scan failed", P.who);
      if (lra_exclusive_scan<uint32_t>(ctx, (long)n_op, head.p, hoff.p)) return P.fail(LRA_ERR_HIP, "%s: a scan failed", P.who);
      if (n_op) {
        hipLaunchKernelGGL(vc_live, dim3(blocks_of(n_op)), dim3(256), 0, st, V);
        hipLaunchKernelGGL(vc_heads, dim3(blocks_of(n_op)), dim3(256), 0, st, V);
      }
      hipLaunchKernelGGL(vc_rec, dim3(blocks_of(n)), dim3(256), 0, st, V);
      LRA_HIP_CHECK(ctx, hipGetLastError());
      if (lra_exclusive_scan<uint32_t>(ctx, (long)n_op, head.p, hoff.p)) return P.fail(LRA_ERR_HIP, "%s: a scan failed", P.who);
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(&n_grp, hoff.p + n_op, 8, hipMemcpyDeviceToHost, st));
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(res, V.F.bad, sizeof res, hipMemcpyDeviceToHost, st));
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(cnt, V.cnt, 8 * N_CNT, hipMemcpyDeviceToHost, st));
      LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
      *ms_ops += T.stop();
      *stop_idx = res[B_STOP];
      const uint64_t lim = std::min<uint64_t>(n, res[B_STOP]);    // (what stands behind the region's end is not this pass's to refuse)
      uint64_t b = NONE; int kind = 0;
      if (lra_vcf_first_bad(res + B_KINDS, lim, &b, &kind)) { memset(cnt, 0, 8 * N_CNT); return P.refuse(b, lra_vcf_bad_text(kind), bad_idx, bad_pos, bad_why); }
    }
    {
      Timer T(st);
      if (!(P.grab(g_op, n_grp + 1) && P.grab(g_m, n_grp + 1) && P.grab(mcnt, n_grp + 1) && P.grab(m_end, n_grp + 1) && P.grab(vkeep, n_grp + 1) && P.grab(voff, n_grp + 1)))
        return P.fail(LRA_ERR_NOMEM, "%s: hipMalloc failed for %llu runs of CIGAR ops", P.who, (unsigned long long)n_grp);
      V.g_op = g_op.p; V.g_m = g_m.p; V.mcnt = mcnt.p; V.m_end = m_end.p; V.vkeep = vkeep.p; V.voff = voff.p; V.n_grp = n_grp;
      if (n_grp) {
        hipLaunchKernelGGL(vc_groups, dim3(blocks_of(n_op)), dim3(256), 0, st, V);
        LRA_HIP_CHECK(ctx, hipGetLastError());
        if (lra_exclusive_scan<uint32_t>(ctx, (long)n_grp, g_m.p, mcnt.p)) return P.fail(LRA_ERR_HIP, "%s: a scan failed", P.who);
        hipLaunchKernelGGL(vc_anchor, dim3(blocks_of(n_grp)), dim3(256), 0, st, V);
        hipLaunchKernelGGL(vc_vkeep, dim3(blocks_of(n_grp)), dim3(256), 0, st, V);
        LRA_HIP_CHECK(ctx, hipGetLastError());
        if (lra_exclusive_scan<uint32_t>(ctx, (long)n_grp, vkeep.p, voff.p)) return P.fail(LRA_ERR_HIP, "%s: a scan failed", P.who);
        LRA_HIP_CHECK(ctx, hipMemcpyAsync(nv, voff.p + n_grp, 8, hipMemcpyDeviceToHost, st));
        if (V.count_small) { LRA_HIP_CHECK(ctx, hipMemcpyAsync(cnt, V.cnt, 8 * N_CNT, hipMemcpyDeviceToHost, st)); }
        LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
      }
      *ms_walk += T.stop();
    }
    if (!*nv) return LRA_OK;
    {
      Timer T(st);
      if (!(P.grab(var, *nv) && (!want_plen || (P.grab(plen, 4 * *nv) && P.grab(poff, 4 * *nv + 1)))))
        return P.fail(LRA_ERR_NOMEM, "%s: hipMalloc failed for %llu variants", P.who, (unsigned long long)*nv);
      V.var = var.p; V.n_var = *nv; V.plen = want_plen ? plen.p : nullptr; V.poff = poff.p;
      hipLaunchKernelGGL(vc_compact, dim3(blocks_of(n_grp)), dim3(256), 0, st, V);
      LRA_HIP_CHECK(ctx, hipGetLastError());
      if (want_plen) {
        if (lra_exclusive_scan<uint32_t>(ctx, (long)(4 * *nv), plen.p, poff.p)) return P.fail(LRA_ERR_HIP, "%s: a scan failed", P.who);
        LRA_HIP_CHECK(ctx, hipMemcpyAsync(total, poff.p + 4 * *nv, 8, hipMemcpyDeviceToHost, st));
        LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
      }
      *ms_lengths += T.stop();
    }
    return LRA_OK;
  }
};

}  // namespace
